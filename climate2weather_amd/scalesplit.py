"""The scale split of an ensemble on the device: *averaged back to the observation's grid, does a member still reproduce what it was
conditioned on, and is the detail it adds below that grid right?*  The sampler is conditioned on ``y = A(x)`` with ``A =
AvgPool2d(s_step) o x[::t_step]`` (``score_fn.PoolStrideOperator``); every other score of the evaluation side judges the members at
the fine grid and mixes the two questions.  For blocks of ``s x s`` cells with block means ``m`` the split is exact:

    sum (x - y)^2 = s^2 (m_x - m_y)^2 + sum ((x - m_x) - (y - m_y))^2

so a member's error divides into what it was given (``coarse``) and what it generated (``detail``), at the observation's scale or at
any other.

**Rows.**  ``d = 0`` is the truth if one is given, then the ``M`` members: ``D = M + 1``, or ``M`` without a truth.

**Block moments** (include/c2w_hip.h: c2w_block_moments).  ``samples (M, T, F, H, W)``, ``truth (T, F, H, W)`` or None, ``s`` with
``H % s == 0`` and ``W % s == 0``; ``h = H / s``, ``w = W / s``.  A float64 or 16-bit input is rounded / widened to fp32 once.  For
each block of each ``(d, t, f)`` plane, cells ``x[r][c]``:

* ``pivot = x[0][0]``, the fp32 value kept as its bits;
* ``e[r][c] = (double)x[r][c] - (double)pivot``, and ``eT`` the same from the truth's block and the truth's pivot;
* column sums, each sequential from ``+0.0`` in row order: ``A_c = sum_r e``, ``Q_c = sum_r e e``, ``X_c = sum_r e eT``; every product
  is rounded on its own, no multiply is fused with an add;
* block sums, each sequential from ``+0.0`` in column order: ``S1 = sum_c A_c``, ``S2 = sum_c Q_c``, ``X = sum_c X_c``;
* ``n`` counts the cells whose fp32 bits are finite (exponent field not all ones: an infinity is invalid).  A block with ``n < s^2``
  holds the canonical NaN in ``S1`` and ``S2``; ``X`` is that NaN if the block or the truth's block is invalid.

Row 0 carries the truth against itself (``X == S2``).  ``sums (D, T, F, NS, h, w)``, ``NS = 3`` with a truth and 2 without.

**Bit for bit on every route.**  That order is the definition: the kernel (csrc/blockmoments.hip: a thread owns 4 adjacent columns of
a block row, the first thread of a block adds its columns), the torch route (``_general``: ``s`` vector adds over the rows, then ``s``
over the columns, in float64) and the NumPy reference of the tests give the same bits.  On the GPU ``s`` in {4, 8, 16, 32} takes the
kernel; every other ``s`` (2 included) and CPU tensors take ``_general``.

**Why the pivot, and why not avg_pool2d.**  An fp32 ``avg_pool2d`` of a pressure-like field (101325 +- 0.5) is off by up to 0.09 at
``s = 16`` and 0.68 at ``s = 32``, more than the field's standard deviation; the sub-grid variance taken from it is wrong by a relative
6.8e-3 and 1.8.  The pivot removes the field's magnitude before any product or sum; csrc/blockmoments_maps.h derives the bound
``2 s 2^-53 sum |e|`` for ``S1`` and ``(2 s + 2) 2^-53 sum |e e|`` for ``S2`` and ``X`` against exact rational arithmetic, and the tests
hold every route to it.

**Scores.**  Float64 tensor algebra on the tables, on the tables' device, with ``N = s^2``, ``V = max(0, S2 - S1 S1 / N)`` (``N`` times
the block's population variance) and ``C = X - S1_x S1_y / N``.  A block invalid in the member or in the truth is left out of that
member's sums and counted.

Out of scope: overlapping or non-square blocks, a spectral (wavelet) split, weights by area, the time aggregation of the observation
beyond ``[::t_step]``.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from . import scale_ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, dense32, member_mean_std, variable_names
from .ensemble_host import on_device as _on_device

DEVICE_SIZES = (4, 8, 16, 32)  # the block sizes the kernel takes (csrc/blockmoments_maps.h: size_ok)
T_STEP = 6                     # the reference's temporal stride of the observation (exp/downscaling.py:129-132)
_EXP = 0x7F800000
_NAN = 0x7FF8000000000000      # the canonical NaN of an invalid block


class BlockMoments(NamedTuple):
    """What ``block_moments`` returns (module docstring)"""
    n: torch.Tensor       # (D, T, F, h, w) int32
    pivot: torch.Tensor   # (D, T, F, h, w) fp32
    sums: torch.Tensor    # (D, T, F, NS, h, w) float64
    s: int
    with_truth: bool


# ---------------------------------------------------------------------------------------------------------------------- the tables

def _finite(rows: torch.Tensor) -> torch.Tensor:
    """fp32 -> bool: the exponent field is not all ones"""
    return (rows.view(torch.int32) & _EXP) != _EXP


def _blocks(a: torch.Tensor, s: int) -> torch.Tensor:
    """``(..., H, W) -> (..., h, w, s, s)``: a view, the block's rows then its columns last"""
    H, W = int(a.shape[-2]), int(a.shape[-1])
    return a.view(*a.shape[:-2], H // s, s, W // s, s).transpose(-3, -2)


def _general(x, y, n, pivot, sums, s: int) -> None:
    """The definition for any block size and any device: x (M, T, F, H, W), y (T, F, H, W) or None dense fp32; the tables as
    ``scale_ops.block_moments`` takes them.  ``s`` vector adds over the rows, then ``s`` over the columns (module docstring)."""
    M, T, F, H, W = (int(v) for v in x.shape)
    with_truth = y is not None
    nan = torch.tensor(_NAN, dtype=torch.int64, device=x.device).view(torch.float64)
    step = chunk_step(8 * F * H * W)
    for t0 in range(0, T, step):
        t1 = min(T, t0 + step)
        yb = _blocks(y[t0:t1], s) if with_truth else None                          # (t, F, h, w, s, s)
        for d in range(int(n.shape[0])):
            xb = yb if (with_truth and d == 0) else _blocks(x[d - 1 if with_truth else d, t0:t1], s)
            P = xb[..., 0, 0]
            e = xb.to(torch.float64) - P.to(torch.float64)[..., None, None]
            count = _finite(xb.contiguous()).sum(dim=(-1, -2), dtype=torch.int32)
            terms = [e, torch.mul(e, e)]
            ok = [count == s * s] * 2
            if with_truth:
                eT = yb.to(torch.float64) - yb[..., 0, 0].to(torch.float64)[..., None, None]
                terms.append(torch.mul(e, eT))
                ok.append(ok[0] & (_finite(yb.contiguous()).sum(dim=(-1, -2), dtype=torch.int32) == s * s))
            n[d, t0:t1], pivot[d, t0:t1] = count, P
            for k, term in enumerate(terms):
                cols = torch.zeros(term.shape[:-2] + (s,), dtype=torch.float64, device=x.device)
                for r in range(s):
                    cols = cols + term[..., r, :]
                total = torch.zeros(term.shape[:-2], dtype=torch.float64, device=x.device)
                for c in range(s):
                    total = total + cols[..., c]
                sums[d, t0:t1, :, k] = torch.where(ok[k], total, nan)


def _launch(x, y, n, pivot, sums, s: int) -> bool:
    M, T, F, H, W = (int(v) for v in x.shape)
    if not scale_ops.supported(H, W, s):
        return False
    return scale_ops.block_moments(x, y, n, pivot, sums, M, T, F, H, W, s)


def _size(s, H: int, W: int) -> int:
    if isinstance(s, bool) or int(s) != s or int(s) < 1:
        raise ValueError(f"s {s!r} must be an integer >= 1")
    if H % int(s) or W % int(s):
        raise ValueError(f"s = {int(s)} must divide H = {H} and W = {W}")
    return int(s)


def block_moments(samples: torch.Tensor, truth: Optional[torch.Tensor] = None, s: int = 16) -> BlockMoments:
    """The block moments of ``samples (M, T, F, H, W)`` and, as row 0, of ``truth (T, F, H, W)`` at block size ``s``.  Any float dtype
    and any strides: a strided or non-fp32 input costs one dense fp32 copy."""
    if truth is not None:
        check_ensemble(samples, truth, members="M >= 1", floating=True)
    elif samples.dim() != 5 or not samples.is_floating_point() or int(samples.shape[0]) < 1:
        raise ValueError(f"samples {tuple(samples.shape)} ({samples.dtype}) must be floating point (M >= 1, T, F, H, W)")
    if truth is not None and truth.device != samples.device:
        raise ValueError(f"truth is on {truth.device}, samples on {samples.device}")
    M, T, F, H, W = (int(v) for v in samples.shape)
    s = _size(s, H, W)
    x, y = dense32(samples), None if truth is None else dense32(truth)
    D, NS, h, w = M + (truth is not None), 3 if truth is not None else 2, H // s, W // s
    n = torch.empty((D, T, F, h, w), dtype=torch.int32, device=x.device)
    pivot = torch.empty((D, T, F, h, w), dtype=torch.float32, device=x.device)
    sums = torch.empty((D, T, F, NS, h, w), dtype=torch.float64, device=x.device)
    if not (_on_device(x) and _launch(x, y, n, pivot, sums, s)):
        _general(x, y, n, pivot, sums, s)
    return BlockMoments(n, pivot, sums, s, truth is not None)


# ---------------------------------------------------------------------------------------------------------------------- the scores

def _need_truth(t: BlockMoments, what: str) -> None:
    if not t.with_truth:
        raise ValueError(f"{what} needs tables with a truth")


def _N(t: BlockMoments) -> float:
    return float(t.s * t.s)


def _V(t: BlockMoments) -> torch.Tensor:
    """``max(0, S2 - S1 S1 / N)`` ``(D, T, F, h, w)``: N times the block's population variance; NaN for an invalid block"""
    S1, S2 = t.sums[:, :, :, 0], t.sums[:, :, :, 1]
    return (S2 - S1 * S1 / _N(t)).clamp(min=0.0)


def coarse(t: BlockMoments) -> torch.Tensor:
    """``(D, T, F, h, w)`` float64: the block means ``pivot + S1 / N`` -- the field at the coarse grid; NaN for an invalid block"""
    return t.pivot.to(torch.float64) + t.sums[:, :, :, 0] / _N(t)


def subgrid_variance(t: BlockMoments) -> torch.Tensor:
    """``(D, T, F, h, w)`` float64: the population variance ``V / N`` of every block's cells about the block's mean"""
    return _V(t) / _N(t)


class _Parts(NamedTuple):
    ok: torch.Tensor   # (M, T, F, h, w) bool: the block is valid in the member and in the truth
    Vx: torch.Tensor   # each (M, T, F, h, w) float64, 0 where not ok
    Vy: torch.Tensor
    C: torch.Tensor
    dm: torch.Tensor   # m_x - m_y


def _parts(t: BlockMoments) -> _Parts:
    N = _N(t)
    full = t.n == t.s * t.s
    ok = full[1:] & full[:1]
    V = _V(t)
    S1 = t.sums[:, :, :, 0]
    C = t.sums[1:, :, :, 2] - S1[1:] * S1[:1] / N
    P = t.pivot.to(torch.float64)
    dm = (P[1:] - P[:1]) + (S1[1:] - S1[:1]) / N
    zero = lambda a: torch.where(ok, a, 0.0)
    return _Parts(ok, zero(V[1:]), zero(V[:1].expand_as(V[1:])), zero(C), zero(dm))


def _over_blocks(a: torch.Tensor) -> torch.Tensor:
    return a.sum(dim=(-1, -2))


def _ratio(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return torch.where(b > 0, a / b, float("nan"))


class VarianceRatio(NamedTuple):
    per_time: torch.Tensor   # (M, T, F) float64
    pooled: torch.Tensor     # (M, F) float64: the sums added over time before the quotient
    blocks: torch.Tensor     # (M, T, F) int64: the blocks that entered
    invalid: torch.Tensor    # (M, T, F) int64: the blocks left out


def _counts(p: _Parts):
    blocks = p.ok.sum(dim=(-1, -2))
    return blocks, p.ok.shape[-1] * p.ok.shape[-2] - blocks


def variance_ratio(t: BlockMoments) -> VarianceRatio:
    """``sum V_member / sum V_truth`` over the blocks: the sub-grid variability a member has against the truth's.  Below 1 means too
    smooth.  NaN where the truth has none."""
    _need_truth(t, "variance_ratio")
    p = _parts(t)
    a, b = _over_blocks(p.Vx), _over_blocks(p.Vy)
    return VarianceRatio(_ratio(a, b), _ratio(a.sum(dim=1), b.sum(dim=1)), *_counts(p))


class ErrorSplit(NamedTuple):
    coarse: torch.Tensor         # (M, T, F) float64: mean squares per cell
    detail: torch.Tensor
    total: torch.Tensor
    coarse_share: torch.Tensor   # coarse / total, NaN where total is 0
    blocks: torch.Tensor         # (M, T, F) int64
    invalid: torch.Tensor


def _split_sums(t: BlockMoments, p: _Parts):
    """the two sums of squares over the blocks ``(M, T, F)`` and the cells they cover"""
    N = _N(t)
    coarse_sum = _over_blocks(N * p.dm * p.dm)
    detail_sum = _over_blocks((p.Vx + p.Vy) - 2.0 * p.C).clamp(min=0.0)
    return coarse_sum, detail_sum, N * _counts(p)[0].to(torch.float64)


def error_split(t: BlockMoments) -> ErrorSplit:
    """The mean squared error of every member against the truth, divided exactly: ``coarse = sum N (m_x - m_y)^2 / cells`` is what
    the member was given, ``detail = max(0, sum (V_x + V_y - 2 C)) / cells`` what it generated, ``total`` their sum -- the mean of
    ``(x - y)^2`` over the cells of the valid blocks."""
    _need_truth(t, "error_split")
    p = _parts(t)
    cs, ds, cells = _split_sums(t, p)
    c, d = cs / cells, ds / cells
    total = c + d
    return ErrorSplit(c, d, total, _ratio(c, total), *_counts(p))


class DetailCorrelation(NamedTuple):
    per_time: torch.Tensor   # (M, T, F) float64
    pooled: torch.Tensor     # (M, F) float64


def _corr(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return torch.where((a > 0) & (b > 0), c / torch.sqrt(a * b), float("nan"))


def detail_correlation(t: BlockMoments) -> DetailCorrelation:
    """``sum C / sqrt(sum V_x sum V_y)``: the correlation of a member's sub-grid detail with the truth's, pooled over the blocks.
    NaN where either has no sub-grid variance."""
    _need_truth(t, "detail_correlation")
    p = _parts(t)
    a, b, c = _over_blocks(p.Vx), _over_blocks(p.Vy), _over_blocks(p.C)
    return DetailCorrelation(_corr(c, a, b), _corr(c.sum(dim=1), a.sum(dim=1), b.sum(dim=1)))


class ObservationResidual(NamedTuple):
    bias: torch.Tensor      # (D, L', F) float64
    rmse: torch.Tensor
    max_abs: torch.Tensor
    blocks: torch.Tensor    # (D, L', F) int64: the valid blocks that entered


def observation_residual(t: BlockMoments, observation: torch.Tensor, t_step: int) -> ObservationResidual:
    """``coarse(t)[:, ::t_step] - observation`` per row, observed time and variable: the consistency of every row with what
    ``condition_on(A=PoolStrideOperator(s, t_step), y=observation)`` was given.  ``observation (L', F, h, w)``, ``L' = ceil(T /
    t_step)``.  An invalid block is left out; NaN where none is left."""
    if isinstance(t_step, bool) or int(t_step) != t_step or int(t_step) < 1:
        raise ValueError(f"t_step {t_step!r} must be an integer >= 1")
    D, T, F, h, w = (int(v) for v in t.n.shape)
    want = (-(-T // int(t_step)), F, h, w)
    if tuple(observation.shape) != want:
        raise ValueError(f"observation {tuple(observation.shape)} must be (ceil(T / t_step), F, h, w) = {want}")
    ok = (t.n == t.s * t.s)[:, ::int(t_step)]
    diff = torch.where(ok, coarse(t)[:, ::int(t_step)] - observation.to(device=t.sums.device, dtype=torch.float64), 0.0)
    blocks = ok.sum(dim=(-1, -2))
    count = blocks.to(torch.float64)
    some = blocks > 0
    nan = float("nan")
    return ObservationResidual(torch.where(some, _over_blocks(diff) / count, nan), torch.where(some, torch.sqrt(_over_blocks(diff * diff) / count), nan),
                               torch.where(some, diff.abs().amax(dim=(-1, -2)), nan), blocks)


class ScaleProfile(NamedTuple):
    scales: tuple
    coarse: torch.Tensor               # each (len(scales), M, F) float64, pooled over time
    detail: torch.Tensor
    variance_ratio: torch.Tensor
    detail_correlation: torch.Tensor


def scale_profile(samples: torch.Tensor, truth: torch.Tensor, scales: Sequence[int] = (2, 4, 8, 16, 32)) -> ScaleProfile:
    """The split at every block size of ``scales``, pooled over time: how the error moves from ``detail`` to ``coarse`` as the blocks
    shrink, and at which scale a member's variability and its correlation with the truth's fall off.  One ``block_moments`` a scale."""
    check_ensemble(samples, truth, members="M >= 1", floating=True)
    rows = []
    for s in scales:
        t = block_moments(samples, truth, s)
        p = _parts(t)
        cs, ds, cells = _split_sums(t, p)
        cells = cells.sum(dim=1)
        rows.append((cs.sum(dim=1) / cells, ds.sum(dim=1) / cells, variance_ratio(t).pooled, detail_correlation(t).pooled))
    return ScaleProfile(tuple(int(s) for s in scales), *(torch.stack([r[k] for r in rows]) for k in range(4)))


# ---------------------------------------------------------------------------------------------------------------------- the report

class ScalesReport(VariableReport):
    """Per variable, as device tensors, ``M`` members over ``L`` times: ``coarse``, ``detail``, ``total``, ``coarse_share``,
    ``variance_ratio``, ``detail_correlation`` ``(M,)`` (pooled over time; ``total`` is the member's mean squared error), their
    ``*_per_time (M, L)``, ``invalid_blocks (M,)`` int64 and, with an observation, ``observation_bias``, ``observation_rmse``,
    ``observation_max_abs (M,)`` (bias and RMSE over all observed blocks, the largest residual) and ``truth_observation_rmse`` (0-d):
    the same of the truth row.  ``s`` and ``t_step`` are attributes."""

    def __init__(self, names, variables, s: int, t_step: Optional[int]):
        super().__init__(names, variables)
        self.s, self.t_step = s, t_step

    def as_dict(self, prefix: str = "scales") -> dict:
        """flat ``{f"{prefix}/{name}/coarse": mean over the members, ..."_std": their population std}``, likewise the other ``(M,)``
        float entries.  For a logger (one device-to-host copy)."""
        if not self.variables:
            return {}
        rows, keys = [], []
        for name, v in self:
            for key in ("coarse", "detail", "total", "coarse_share", "variance_ratio", "detail_correlation", "observation_bias", "observation_rmse",
                        "observation_max_abs"):
                if key in v:
                    rows.append(v[key])
                    keys.append(f"{prefix}/{name}/{key}")
        return member_mean_std(rows, keys)


def scales_report(samples: torch.Tensor, truth: torch.Tensor, observation: Optional[torch.Tensor] = None, s: Optional[int] = None,
                  t_step: Optional[int] = None, names: Optional[Sequence[str]] = None) -> ScalesReport:
    """The scale split of an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)``, per variable, and -- with the
    ``observation (L', F, h, w)`` the sampler was conditioned on -- every member's consistency with it.  ``s`` defaults to ``H // h``
    of the observation, else 16; ``t_step`` to 1 if the observation has every time, else the reference's 6.  ``names``: one per
    variable, default ``var0 ...``."""
    check_ensemble(samples, truth, time="L", members="M >= 1", floating=True)
    M, L, F, H, W = (int(v) for v in samples.shape)
    names = variable_names(names, F)
    if observation is not None:
        if observation.dim() != 4 or int(observation.shape[-2]) < 1 or H % int(observation.shape[-2]):
            raise ValueError(f"observation {tuple(observation.shape)} must be (L', F, h, w) with h a divisor of H = {H}")
        if s is None:
            s = H // int(observation.shape[-2])
        if t_step is None:
            t_step = 1 if int(observation.shape[0]) == L else T_STEP
    t = block_moments(samples, truth, 16 if s is None else s)
    split, ratio, corr = error_split(t), variance_ratio(t), detail_correlation(t)
    p = _parts(t)
    cs, ds, cells = _split_sums(t, p)
    cells = cells.sum(dim=1)
    pc, pd = cs.sum(dim=1) / cells, ds.sum(dim=1) / cells                        # (M, F)
    invalid = split.invalid.sum(dim=1)
    res = None if observation is None else observation_residual(t, observation, t_step)
    variables = []
    for f in range(F):
        v = dict(coarse=pc[:, f], detail=pd[:, f], total=pc[:, f] + pd[:, f], coarse_share=_ratio(pc[:, f], pc[:, f] + pd[:, f]),
                 variance_ratio=ratio.pooled[:, f], detail_correlation=corr.pooled[:, f], coarse_per_time=split.coarse[:, :, f],
                 detail_per_time=split.detail[:, :, f], total_per_time=split.total[:, :, f], coarse_share_per_time=split.coarse_share[:, :, f],
                 variance_ratio_per_time=ratio.per_time[:, :, f], detail_correlation_per_time=corr.per_time[:, :, f], invalid_blocks=invalid[:, f])
        if res is not None:
            count = res.blocks[:, :, f].to(torch.float64)                         # (D, L')
            done = torch.where(count > 0, res.bias[:, :, f], 0.0), torch.where(count > 0, res.rmse[:, :, f], 0.0)
            every = count.sum(dim=1)
            bias, rmse = (done[0] * count).sum(dim=1) / every, torch.sqrt((done[1] * done[1] * count).sum(dim=1) / every)
            worst = torch.where(count > 0, res.max_abs[:, :, f], 0.0).amax(dim=1)
            v.update(observation_bias=bias[1:], observation_rmse=rmse[1:], observation_max_abs=worst[1:], truth_observation_rmse=rmse[0])
        variables.append(v)
    return ScalesReport(names, variables, t.s, None if observation is None else int(t_step))
