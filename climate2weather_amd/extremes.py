"""Extremes of an ensemble on the device: *what does the tail do?*  Every other score of the evaluation side is an average over the
whole distribution (``crps``, ``marginals``, ``quantiles``) or needs a threshold chosen in advance (``events``, ``spells``,
``objects``).  This module takes the block maxima (or minima) of every series -- the largest gust of a day, the lowest pressure of a
month --, their sample L-moments, a GEV fitted to them per cell and the return levels of that fit, for the members and for the truth
alike.  Ten years of hourly fields do not arrive at once: ``ExtremeAccumulator.update`` takes them in calls of any length.

**Rows.**  ``d = 0`` is the truth if one is given, then the ``M`` members: ``D = M + 1``, or ``M`` without a truth.

**Series, direction, blocks.**  A series is one ``(d, f, cell)`` over time.  ``direction`` is ``"max"`` or ``"min"``, one for all
variables or one per variable (``dir[F]``: 1 maxima, 0 minima).  Block ``b`` holds the absolute hours ``[b block, (b + 1) block)``,
hour 0 being the first plane of the first update.

**Block extreme** (include/c2w_hip.h: c2w_block_extremes_update).  The extreme of a block is taken in the total order of the quantile
key on the fp32 bit patterns -- a float64 or 16-bit input is rounded / widened to fp32 once --, so ``-0.0 < +0.0`` and the infinities
are ordinary values.  NaN hours are skipped and counted per ``(d, f)`` in ``invalid`` (int64); a block whose hours are all NaN has the
extreme NaN (the one pattern ``0x7FC00000``).  Everything is integer compares on keys: the tables are the same **bit for bit** on
every route and for every cut of the time axis into updates.

**Sample L-moments** of the ``n`` block extremes of a series (include/c2w_hip.h: c2w_lmoments); NaN extremes are dropped, ``n' <= n``
remain, ``x_(0) <= ... <= x_(n' - 1)``:

    b_r = (1 / n') sum_j [j (j - 1) .. (j - r + 1) / ((n' - 1) .. (n' - r))] x_(j)
    l1 = b0     l2 = 2 b1 - b0     l3 = 6 b2 - 6 b1 + b0     l4 = 20 b3 - 30 b2 + 12 b1 - b0

-- ``scipy.stats.lmoment(..., standardize=False)``.  All in float64 on exactly converted fp32 values: every ``x_(j)`` is first reduced
by the middle order statistic ``x_(n' // 2)`` (the pivot; the weights of ``l2 .. l4`` sum to zero, only ``l1`` adds it back), the
integer weights ``j (j - 1) ..`` multiply the reduced values, the sums run in ascending ``j``, one division by the exact integer
``n' (n' - 1) .. (n' - r)`` follows, no multiply is fused with an add.  ``l_r`` is NaN where ``n' < r``.  csrc/extremes_maps.h derives
the bound ``c_r(n') 2^-53 sum_j |x_(j) - pivot|`` (plus one rounding of ``l1``) the tests hold every route to.

**GEV by L-moments**, Hosking's parametrisation ``F(x) = exp(-(1 - k (x - xi) / alpha)^(1 / k))``: the shape ``k`` is scipy's
``genextreme`` ``c``; ``k > 0`` is bounded above, ``k < 0`` heavy-tailed, ``k = 0`` Gumbel.  With ``t3 = l3 / l2`` the start
``c = 2 / (3 + t3) - ln 2 / ln 3``, ``k0 = 7.8590 c + 2.9554 c^2`` (recalled from Hosking & Wallis; README, statement 16) is followed
by **six fixed Newton steps** on ``g(k) = 2 (1 - 3^-k) / (1 - 2^-k) - 3 - t3`` -- the approximation alone is off by up to 0.08 in
``k`` and is not the definition.  Then ``alpha = l2 k / ((1 - 2^-k) Gamma(1 + k))`` and ``xi = l1 - alpha (1 - Gamma(1 + k)) / k``.
Every quotient that is 0/0 at ``k = 0`` goes through ``expm1`` / ``lgamma`` (``lgamma(1 + k)`` by its series below ``|k| = 1/32``,
where ``1 + k`` would round ``k`` away), so ``k -> 0`` is continuous; exactly 0 takes the Gumbel limits ``ln 3 / ln 2``,
``1 / ln 2``, Euler's constant and ``-ln(-ln p)``.  The return level of period ``R`` blocks is the quantile at ``p = 1 - 1 / R``.  A
cell with ``l2 <= 0``, ``n' < 3`` or ``|t3| >= 1`` gets NaN parameters and is counted in ``unfitted``.

On the GPU ``H W`` a multiple of 4, ``block <= 2^20`` and ``max_blocks <= 4096`` take the streaming kernel, and ``n <= 64`` blocks
the L-moment kernel (csrc/extremes.hip).  Everything else and CPU tensors take the same numbers from torch (``_general*``): block
extremes by integer ``amax`` of the keys over reshaped blocks, ``torch.sort`` for the moments.  The fit, the return levels and the
scores are float64 tensor algebra on the maps and stay on the device.  Nothing here synchronises.

Out of scope: peaks over threshold / GPD, the hour at which the extreme occurred, non-stationary fits, bootstrap confidence intervals,
``n > 64`` blocks on the device (the general route serves them; a ten-year monthly series is 120 blocks -- the next step).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import extreme_ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, datasets, dense32, member_mean_std, variable_names
from .ensemble_host import on_device as _on_device

MAX_CALL = 1 << 20         # hours one launch takes (csrc/extremes_maps.h: MAX_T); a longer update is walked in parts
NONE = 0                   # the key "no value yet"
NAN_BITS = 0x7FC00000      # the extreme of a block without a value
_ALL, _TOP = 0xFFFFFFFF, 0x80000000
LN2, LN3, EULER = math.log(2.0), math.log(3.0), 0.5772156649015329
# zeta(2) .. zeta(13): lgamma(1 + k) = -EULER k + sum_{n >= 2} (-1)^n zeta(n) k^n / n
_ZETA = (1.6449340668482264, 1.2020569031595942, 1.0823232337111382, 1.0369277551433699, 1.0173430619844491, 1.0083492773819228,
         1.0040773561979443, 1.0020083928260822, 1.0009945751278181, 1.0004941886041195, 1.0002460865533080, 1.0001227133475785)
PIT_BINS = 10


class ExtremeTables(NamedTuple):
    """What ``ExtremeAccumulator.tables`` returns (module docstring)"""
    extremes: torch.Tensor  # (D, F, n_blocks, H, W) fp32
    n_blocks: int
    open_hours: int         # hours seen of the block that is not complete (0: none)
    invalid: torch.Tensor   # (D, F) int64


# ---------------------------------------------------------------------------------------------------------------------- keys

def _unsigned(a: torch.Tensor) -> torch.Tensor:
    """int32 bit patterns as int64 numbers 0 .. 2^32 - 1"""
    return a.to(torch.int64) & _ALL


def _signed(a: torch.Tensor) -> torch.Tensor:
    """int64 numbers 0 .. 2^32 - 1 as int32 bit patterns"""
    return torch.where(a >= _TOP, a - (1 << 32), a).to(torch.int32)


def _dkeys(rows: torch.Tensor, flip: torch.Tensor):
    """fp32 ``rows (..., F, c)`` -> (the directed keys as int64, the NaN mask): csrc/extremes_maps.h::dkey_of"""
    bits = _unsigned(rows.view(torch.int32))
    key = bits ^ torch.where(bits >= _TOP, _ALL, _TOP)
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    return torch.where(nan, NONE, key ^ flip), nan


def _values(dkey: torch.Tensor, flip: torch.Tensor) -> torch.Tensor:
    """directed keys ``(..., F, c)`` int64 -> the fp32 values: csrc/extremes_maps.h::extreme_bits"""
    key = dkey ^ flip
    bits = key ^ torch.where(key >= _TOP, _TOP, _ALL)
    return _signed(torch.where(dkey == NONE, NAN_BITS, bits)).view(torch.float32)


def _flip(dirn: torch.Tensor) -> torch.Tensor:
    return torch.where(dirn != 0, 0, _ALL).to(torch.int64).view(-1, 1)


def _direction(direction, F: int, device) -> torch.Tensor:
    """``"max"`` / ``"min"``, one or one per variable -> int32 ``(F,)``, 1 for maxima"""
    names = [direction] * F if isinstance(direction, str) else list(direction)
    if len(names) != F or any(n not in ("max", "min") for n in names):
        raise ValueError(f"direction {direction!r} must be 'max' or 'min', or one of them per variable ({F})")
    return torch.tensor([1 if n == "max" else 0 for n in names], dtype=torch.int32, device=device)


# ---------------------------------------------------------------------------------------------------------------------- one call

def _general(x, y, dirn, open_keys, table, invalid, block: int, t_abs: int) -> None:
    """The definition for any shape and any device: the keys of the call's hours, an integer ``amax`` over the rest of the open
    block, over the whole blocks behind it (reshaped to ``(D, blocks, block, F, cells)``) and over the hours that remain, the carried
    key joined to the first.  x (M, T, F, hw), y (T, F, hw) or None; the rest as ``extreme_ops.block_extremes_update`` takes it."""
    M, T, F, hw = (int(s) for s in x.shape)
    D = int(open_keys.shape[0])
    if T == 0:
        return
    flip = _flip(dirn)
    b0 = t_abs // block
    head = min(T, block - t_abs % block)            # the hours that go to the block open at the start
    whole = (T - head) // block                     # the blocks that lie in the call from their first hour to their last
    tail = head + whole * block                     # behind them: the hours of a block the call does not end
    nb = 1 + whole + (1 if tail < T else 0)
    n_closed = (t_abs + T) // block - b0
    step = chunk_step(D * T * F)
    for c0 in range(0, hw, step):
        c1 = min(hw, c0 + step)
        rows = x[..., c0:c1] if y is None else torch.cat([y[None, ..., c0:c1], x[..., c0:c1]])          # (D, T, F, c)
        k, nan = _dkeys(rows, flip)
        invalid += nan.sum(dim=(1, 3))
        parts = [k[:, :head].amax(dim=1, keepdim=True)]
        if whole:
            parts.append(k[:, head:tail].reshape(D, whole, block, F, c1 - c0).amax(dim=2))
        if tail < T:
            parts.append(k[:, tail:].amax(dim=1, keepdim=True))
        m = torch.cat(parts, dim=1)                                                                       # (D, nb, F, c)
        m[:, 0] = torch.maximum(m[:, 0], _unsigned(open_keys[:, :, c0:c1]))
        if n_closed:
            table[:, :, b0:b0 + n_closed, c0:c1] = _values(m[:, :n_closed], flip).permute(0, 2, 1, 3)
        open_keys[:, :, c0:c1] = _signed(m[:, nb - 1]) if nb > n_closed else 0


def _launch(x, y, dirn, open_keys, table, invalid, block: int, t_abs: int) -> bool:
    M, T, F, hw = (int(s) for s in x.shape)
    B = int(table.shape[2])
    if not extreme_ops.update_supported(hw, block, B):
        return False
    return extreme_ops.block_extremes_update(x, y, dirn, open_keys, table, invalid, M, T, F, hw, block, B, t_abs)


# ---------------------------------------------------------------------------------------------------------------------- the accumulator

def _count(value, name: str, low: int) -> int:
    if isinstance(value, bool) or int(value) != value or int(value) < low:
        raise ValueError(f"{name} {value!r} must be an integer >= {low}")
    return int(value)


class ExtremeAccumulator:
    """Block extremes of ``M`` members (and the truth) of ``F`` variables on ``H x W`` cells, carried from update to update:

        acc = ExtremeAccumulator(M, F, H, W, block=24, direction="max", max_blocks=3660, device=samples.device)
        for samples, truth in calls:           # (M, T, F, H, W), (T, F, H, W); any T >= 0
            acc.update(samples, truth)
        tables = acc.tables()

    ``block``: the hours of a block; ``direction`` as in the module docstring; ``with_truth=False``: the rows are the members alone
    and ``update`` takes no truth; ``max_blocks``: the blocks the table has room for.  The memory is that of the table,
    ``4 D F max_blocks H W`` bytes, and of one key per series."""

    def __init__(self, M: int, F: int, H: int, W: int, block: int, direction="max", *, with_truth: bool = True, max_blocks: int, device=None):
        self.M, self.F, self.H, self.W = _count(M, "M", 1), _count(F, "F", 1), _count(H, "H", 1), _count(W, "W", 1)
        self.block, self.max_blocks = _count(block, "block", 1), _count(max_blocks, "max_blocks", 1)
        self.with_truth = bool(with_truth)
        self.device = torch.device("cpu" if device is None else device)
        self.dirn = _direction(direction, self.F, self.device)
        self.D = self.M + (1 if self.with_truth else 0)
        D, hw = self.D, self.H * self.W
        self.open = torch.zeros((D, self.F, hw), dtype=torch.int32, device=self.device)
        self.table = torch.full((D, self.F, self.max_blocks, hw), float("nan"), dtype=torch.float32, device=self.device)
        self.invalid = torch.zeros((D, self.F), dtype=torch.int64, device=self.device)
        self.n_times = 0

    def update(self, samples: torch.Tensor, truth: Optional[torch.Tensor] = None) -> "ExtremeAccumulator":
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
        if (self.n_times + T) // self.block > self.max_blocks:
            raise ValueError(f"{self.n_times} + {T} hours complete {(self.n_times + T) // self.block} blocks of {self.block}: "
                             f"over max_blocks = {self.max_blocks}")
        for s in range(0, T, MAX_CALL):
            self._call(samples[:, s:s + MAX_CALL], None if truth is None else truth[s:s + MAX_CALL])
        return self

    def _call(self, samples, truth) -> None:
        x, y, _ = datasets(samples, truth)
        args = (x, y, self.dirn, self.open, self.table, self.invalid, self.block, self.n_times)
        if not (_on_device(x) and _launch(*args)):
            _general(*args)
        self.n_times += int(x.shape[1])

    def tables(self, partial: str = "drop") -> ExtremeTables:
        """The extremes of the complete blocks, as a copy; ``partial="keep"`` adds the extreme of the hours seen of an incomplete last
        block, ``"drop"`` (the default, as incomplete years are left out of annual maxima) leaves it out.  The state is left alone."""
        if partial not in ("drop", "keep"):
            raise ValueError(f"partial {partial!r} must be 'drop' or 'keep'")
        n, open_hours = self.n_times // self.block, self.n_times % self.block
        ext = self.table[:, :, :n]
        if partial == "keep" and open_hours:
            ext = torch.cat([ext, _values(_unsigned(self.open), _flip(self.dirn))[:, :, None]], dim=2)
            n += 1
        else:
            ext = ext.clone()
        return ExtremeTables(ext.view(self.D, self.F, n, self.H, self.W), n, open_hours, self.invalid.clone())

    def state_dict(self) -> dict:
        """everything a later ``load_state_dict`` needs to go on where this run stopped (copies)"""
        return dict(open=self.open.clone(), table=self.table.clone(), invalid=self.invalid.clone(), n_times=self.n_times, block=self.block,
                    max_blocks=self.max_blocks, direction=self.dirn.clone())

    def load_state_dict(self, sd: dict) -> "ExtremeAccumulator":
        for key in ("block", "max_blocks"):
            if int(sd[key]) != getattr(self, key):
                raise ValueError(f"{key} {sd[key]} of the state differs from this accumulator's {getattr(self, key)}")
        if not torch.equal(sd["direction"].to(self.device), self.dirn):
            raise ValueError("the directions of the state differ from this accumulator's")
        for key in ("open", "table", "invalid"):
            mine = getattr(self, key)
            if tuple(sd[key].shape) != tuple(mine.shape):
                raise ValueError(f"{key} {tuple(sd[key].shape)} of the state must be {tuple(mine.shape)}")
        for key in ("open", "table", "invalid"):
            setattr(self, key, sd[key].to(device=self.device, dtype=getattr(self, key).dtype).clone().contiguous())
        self.n_times = int(sd["n_times"])
        return self


def block_extremes(samples: torch.Tensor, truth: Optional[torch.Tensor], block: int, direction="max", partial: str = "drop") -> ExtremeTables:
    """One update plus ``tables()``: ``samples (M, T, F, H, W)``, ``truth (T, F, H, W)`` or None"""
    if samples.dim() != 5:
        raise ValueError(f"samples {tuple(samples.shape)} must be (M, T, F, H, W)")
    M, T, F, H, W = (int(s) for s in samples.shape)
    block = _count(block, "block", 1)
    acc = ExtremeAccumulator(M, F, H, W, block, direction, with_truth=truth is not None, max_blocks=max(1, T // block), device=samples.device)
    return acc.update(samples, truth).tables(partial)


# ---------------------------------------------------------------------------------------------------------------------- L-moments

def _general_lmoments(table: torch.Tensor, lmom: torch.Tensor, n_valid: torch.Tensor) -> None:
    """The arithmetic of csrc/extremes_maps.h in float64 torch, for any ``n``: ``table (R, n, hw)`` fp32 -> ``lmom (R, 4, hw)``,
    ``n_valid (R, hw)``.  The sums run over ``j`` one after the other, as the kernel's do."""
    R, n, hw = (int(s) for s in table.shape)
    step = chunk_step(8 * n * hw)
    inf = float("inf")
    for r0 in range(0, R, step):
        t = table[r0:r0 + step]
        nan = torch.isnan(t)
        nv = (~nan).sum(dim=1)                                                       # (r, hw)
        s = torch.where(nan, inf, t).sort(dim=1).values.to(torch.float64)             # pads and NaNs behind the n' values
        p = s.gather(1, (nv // 2).clamp(max=n - 1)[:, None])[:, 0]
        S = [torch.zeros_like(p) for _ in range(4)]
        for j in range(n):
            e = torch.where(j < nv, s[:, j] - p, 0.0)
            S[0] = S[0] + e
            S[1] = S[1] + float(j) * e
            S[2] = S[2] + float(j * (j - 1)) * e
            S[3] = S[3] + float(j * (j - 1) * (j - 2)) * e
        m = nv.to(torch.int64)
        d = [m, m * (m - 1), m * (m - 1) * (m - 2), m * (m - 1) * (m - 2) * (m - 3)]
        b = [S[r] / d[r].to(torch.float64) for r in range(4)]
        l = [p + b[0], 2.0 * b[1] - b[0], (6.0 * b[2] - 6.0 * b[1]) + b[0], ((20.0 * b[3] - 30.0 * b[2]) + 12.0 * b[1]) - b[0]]
        for r in range(4):
            lmom[r0:r0 + step, r] = torch.where(nv >= r + 1, l[r], float("nan"))
        n_valid[r0:r0 + step] = nv.to(torch.int32)


def _launch_lmoments(table, lmom, n_valid) -> bool:
    R, n, hw = (int(s) for s in table.shape)
    if not extreme_ops.lmoments_supported(hw, n):
        return False
    return extreme_ops.lmoments(table, lmom, n_valid, R, n, hw)


def lmoments(extremes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``extremes (..., n, H, W)`` -> ``(lmom (..., 4, H, W) float64, n_valid (..., H, W) int32)``: the sample L-moments ``l1 .. l4`` of
    every cell's non-NaN block extremes and their number ``n'``; ``l_r`` is NaN where ``n' < r``"""
    if extremes.dim() < 3 or int(extremes.shape[-3]) < 1 or not extremes.is_floating_point():
        raise ValueError(f"extremes {tuple(extremes.shape)} ({extremes.dtype}) must be floating point (..., n >= 1, H, W)")
    lead = tuple(extremes.shape[:-3])
    n, H, W = (int(s) for s in extremes.shape[-3:])
    R = math.prod(lead)
    table = dense32(extremes).view(R, n, H * W)
    lmom = torch.empty((R, 4, H * W), dtype=torch.float64, device=table.device)
    n_valid = torch.empty((R, H * W), dtype=torch.int32, device=table.device)
    if R and not (_on_device(table) and _launch_lmoments(table, lmom, n_valid)):
        _general_lmoments(table, lmom, n_valid)
    return lmom.view(lead + (4, H, W)), n_valid.view(lead + (H, W))


def _lmom(lmom: torch.Tensor) -> torch.Tensor:
    if lmom.dim() < 3 or int(lmom.shape[-3]) != 4:
        raise ValueError(f"lmom {tuple(lmom.shape)} must be (..., 4, H, W)")
    return lmom.to(torch.float64)


def lmoment_ratios(lmom: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``lmom (..., 4, H, W)`` -> ``(t, t3, t4)``, each ``(..., H, W)`` float64: the L-CV ``l2 / l1``, the L-skewness ``l3 / l2`` and
    the L-kurtosis ``l4 / l2``"""
    l = _lmom(lmom)
    l1, l2, l3, l4 = l.unbind(-3)
    return l2 / l1, l3 / l2, l4 / l2


# ---------------------------------------------------------------------------------------------------------------------- the GEV

def _lgamma1p(k: torch.Tensor) -> torch.Tensor:
    """``lgamma(1 + k)`` without rounding ``k`` away in ``1 + k``: the series in ``zeta(n)`` below ``|k| = 1/32`` (the term after the
    last is under 1e-22 there)"""
    small = k.abs() < 1.0 / 32
    ks = torch.where(small, k, torch.zeros_like(k))
    series = torch.zeros_like(k)
    for i in range(len(_ZETA) - 1, -1, -1):   # Horner, n = 13 .. 2
        n = i + 2
        series = series * ks + (_ZETA[i] / n if n % 2 == 0 else -_ZETA[i] / n)
    series = (series * ks - EULER) * ks
    return torch.where(small, series, torch.lgamma(1.0 + torch.where(small, torch.ones_like(k), k)))


def _shape_from_t3(t3: torch.Tensor) -> torch.Tensor:
    """Hosking's start and six Newton steps on ``g(k) = 2 (1 - 3^-k) / (1 - 2^-k) - 3 - t3``.  ``g' = 2 r (ln3 / expm1(k ln3) -
    ln2 / expm1(k ln2))`` with ``r`` the quotient; the bracket is the difference of two numbers near ``1 / k`` and is taken from its
    series below ``|k| = 1e-3`` -- the derivative only steers the steps, the root is ``g``'s."""
    c = 2.0 / (3.0 + t3) - LN2 / LN3
    k = 7.8590 * c + 2.9554 * c * c
    for _ in range(6):
        zero, small = k == 0, k.abs() < 1e-3
        kq = torch.where(zero, torch.ones_like(k), k)
        r = torch.where(zero, LN3 / LN2, torch.expm1(-kq * LN3) / torch.expm1(-kq * LN2))
        kd = torch.where(small, torch.ones_like(k), k)
        bracket = torch.where(small, -(LN3 - LN2) / 2 + k * (LN3 ** 2 - LN2 ** 2) / 12 - k ** 3 * (LN3 ** 4 - LN2 ** 4) / 720,
                              LN3 / torch.expm1(kd * LN3) - LN2 / torch.expm1(kd * LN2))
        k = k - (2.0 * r - 3.0 - t3) / (2.0 * r * bracket)
    return k


def gev_fit(lmom: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``lmom (..., 4, H, W)`` -> ``(xi, alpha, k, unfitted)``: location, scale and shape ``(..., H, W)`` float64 of the GEV whose first
    three L-moments are the cell's, and ``unfitted (...)`` int64, the cells with ``l2 <= 0``, ``n' < 3`` (``l3`` is NaN) or
    ``|t3| >= 1``, whose parameters are NaN"""
    l = _lmom(lmom)
    l1, l2, l3, _ = l.unbind(-3)
    t3 = l3 / l2
    fitted = (l2 > 0) & (t3.abs() < 1)
    k = _shape_from_t3(torch.where(fitted, t3, torch.zeros_like(t3)))
    zero = k == 0
    kq = torch.where(zero, torch.ones_like(k), k)
    lg = _lgamma1p(k)
    alpha = l2 * torch.where(zero, 1.0 / LN2, kq / -torch.expm1(-kq * LN2)) / torch.exp(lg)
    xi = l1 - alpha * torch.where(zero, EULER, -torch.expm1(lg) / kq)
    nan = torch.full_like(k, float("nan"))
    return torch.where(fitted, xi, nan), torch.where(fitted, alpha, nan), torch.where(fitted, k, nan), (~fitted).sum(dim=(-1, -2))


def _params(xi, alpha, k):
    if not (tuple(xi.shape) == tuple(alpha.shape) == tuple(k.shape)):
        raise ValueError(f"xi {tuple(xi.shape)}, alpha {tuple(alpha.shape)} and k {tuple(k.shape)} must have one shape")
    return xi.to(torch.float64), alpha.to(torch.float64), k.to(torch.float64)


def gev_return_level(xi: torch.Tensor, alpha: torch.Tensor, k: torch.Tensor, periods: Sequence[float]) -> torch.Tensor:
    """``xi, alpha, k (..., H, W)`` and ``P`` periods ``R > 1`` in blocks -> ``(..., P, H, W)`` float64: the quantile at
    ``p = 1 - 1 / R``, ``xi + alpha (1 - (-ln p)^k) / k``"""
    xi, alpha, k = _params(xi, alpha, k)
    periods = [float(R) for R in periods]
    if xi.dim() < 2 or not periods or any(not R > 1.0 for R in periods):
        raise ValueError(f"periods {periods} must be at least one R > 1, the parameters {tuple(xi.shape)} (..., H, W)")
    ly = torch.tensor([math.log(-math.log1p(-1.0 / R)) for R in periods], dtype=torch.float64, device=xi.device).view(-1, 1, 1)  # ln(-ln p)
    xi, alpha, k = xi.unsqueeze(-3), alpha.unsqueeze(-3), k.unsqueeze(-3)
    zero = k == 0
    kq = torch.where(zero, torch.ones_like(k), k)
    return xi + alpha * torch.where(zero, -ly, -torch.expm1(kq * ly) / kq)


def gev_cdf(x: torch.Tensor, xi: torch.Tensor, alpha: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """``F(x) = exp(-(1 - k (x - xi) / alpha)^(1 / k))`` in float64, ``x`` broadcast against the parameters; 0 below the support
    (``k < 0``) and 1 above it (``k > 0``); NaN where ``x`` or a parameter is"""
    xi, alpha, k = _params(xi, alpha, k)
    z = (x.to(torch.float64) - xi) / alpha
    k = k.expand_as(z)
    zero = k == 0
    kq = torch.where(zero, torch.ones_like(k), k)
    inside = 1.0 - kq * z > 0
    w = torch.where(zero, -z, torch.log1p(torch.where(inside, -kq * z, torch.zeros_like(z))) / kq)
    F = torch.exp(-torch.exp(w))
    F = torch.where(zero | inside, F, (k > 0).to(torch.float64))
    return torch.where(torch.isnan(z) | torch.isnan(k), torch.full_like(F, float("nan")), F)


# ---------------------------------------------------------------------------------------------------------------------- the algebra

def _number(n: int, like: torch.Tensor) -> torch.Tensor:
    return torch.full((), float(n), dtype=torch.float64, device=like.device)


def _against_truth(a: torch.Tensor, lead: int, name: str) -> torch.Tensor:
    """``a (D >= 2, ...)`` with at least ``lead`` axes, row 0 the truth -> members minus truth"""
    if a.dim() < lead or int(a.shape[0]) < 2:
        raise ValueError(f"{name} {tuple(a.shape)} must have {lead} axes, the first D >= 2 rows with row 0 the truth")
    a = a.to(torch.float64)
    return a[1:] - a[:1]


def _pooled(diff: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """bias and RMSE over the cells (the last two axes) that are not NaN; NaN where none is"""
    ok = ~torch.isnan(diff)
    d = torch.where(ok, diff, torch.zeros_like(diff))
    cells = ok.sum(dim=(-1, -2)).to(torch.float64)
    return d.sum(dim=(-1, -2)) / cells, ((d * d).sum(dim=(-1, -2)) / cells).sqrt()


def mean_extreme_error(lmom: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``lmom (D, F, 4, H, W)`` with row 0 the truth -> ``(bias, rmse)``, each ``(D - 1, F)`` float64, of each member's map of the mean
    block extreme ``l1`` against the truth's, over the cells"""
    return _pooled(_against_truth(_lmom(lmom), 5, "lmom")[:, :, 0])


def return_level_error(levels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``levels (D, F, P, H, W)`` with row 0 the truth -> ``(bias, rmse, member_mean)``: bias and RMSE ``(D - 1, F, P)`` float64 of each
    member's return-level map against the truth's, pooled over the cells where both are fitted, and the mean map of the members
    ``(F, P, H, W)``"""
    diff = _against_truth(levels, 5, "levels")
    bias, rmse = _pooled(diff)
    return bias, rmse, levels[1:].to(torch.float64).sum(dim=0) / _number(int(levels.shape[0]) - 1, levels)


def lmoment_ratio_error(lmom: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``lmom (D, F, 4, H, W)`` with row 0 the truth -> ``(bias, rmse)``, each ``(D - 1, F, 3)`` float64, of each member's maps of
    ``t, t3, t4`` against the truth's, over the cells where both are numbers"""
    if lmom.dim() != 5:
        raise ValueError(f"lmom {tuple(lmom.shape)} must be (D >= 2, F, 4, H, W), row 0 the truth")
    return _pooled(_against_truth(torch.stack(lmoment_ratios(lmom), dim=2), 5, "lmom"))


def regional_lmoments(lmom: torch.Tensor, n_valid: torch.Tensor) -> torch.Tensor:
    """``lmom (..., 4, H, W)``, ``n_valid (..., H, W)`` -> ``(..., 3)`` float64: the ``n'``-weighted means over the cells of ``t, t3,
    t4`` (the regional L-moment ratios of an index-flood analysis); a cell whose ratio is NaN has no weight in it"""
    ratios = torch.stack(lmoment_ratios(lmom), dim=-3)                                  # (..., 3, H, W)
    if tuple(n_valid.shape) != tuple(ratios.shape[:-3] + ratios.shape[-2:]):
        raise ValueError(f"n_valid {tuple(n_valid.shape)} must be {tuple(ratios.shape[:-3] + ratios.shape[-2:])}, lmom's without the moments")
    ok = ~torch.isnan(ratios)
    w = torch.where(ok, n_valid.to(torch.float64).unsqueeze(-3).expand_as(ratios), torch.zeros_like(ratios))
    return (w * torch.where(ok, ratios, torch.zeros_like(ratios))).sum(dim=(-1, -2)) / w.sum(dim=(-1, -2))


def gev_pit(extremes: torch.Tensor, xi: torch.Tensor, alpha: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """``extremes (D, F, n, H, W)`` with row 0 the truth and the fits ``(D, F, H, W)`` -> int64 ``(D - 1, F, 10)``: the truth's block
    extremes binned by their probability under each member's fitted GEV, ``min(floor(10 F(x)), 9)``.  A flat histogram means calibrated
    tails.  A NaN extreme or an unfitted cell is in no bin."""
    if extremes.dim() != 5 or int(extremes.shape[0]) < 2 or tuple(xi.shape) != tuple(extremes.shape[:2] + extremes.shape[3:]):
        raise ValueError(f"extremes {tuple(extremes.shape)} must be (D >= 2, F, n, H, W), row 0 the truth, and the fits {tuple(xi.shape)} (D, F, H, W)")
    D, F = int(extremes.shape[0]), int(extremes.shape[1])
    u = gev_cdf(extremes[:1], xi[1:, :, None], alpha[1:, :, None], k[1:, :, None])     # (M, F, n, H, W)
    ok = ~torch.isnan(u)
    bins = torch.where(ok, (u * PIT_BINS).floor().clamp(0, PIT_BINS - 1), torch.zeros_like(u)).to(torch.int64)
    row = torch.arange((D - 1) * F, device=u.device).view(D - 1, F, 1, 1, 1)
    counts = torch.zeros(((D - 1) * F * PIT_BINS,), dtype=torch.int64, device=u.device)
    counts.scatter_add_(0, (row * PIT_BINS + bins).reshape(-1), ok.to(torch.int64).reshape(-1))
    return counts.view(D - 1, F, PIT_BINS)


# ---------------------------------------------------------------------------------------------------------------------- the report

class ExtremesReport(VariableReport):
    """Per variable, as device tensors, ``D`` rows (0 the truth), ``P`` periods: ``direction`` (1 maxima), ``periods (P,)``,
    ``n_blocks``, ``regional (D, 3)`` (``t, t3, t4``), ``mean_extreme_bias``, ``mean_extreme_rmse (M,)``, ``ratio_bias``,
    ``ratio_rmse (M, 3)``, ``return_level_bias``, ``return_level_rmse (M, P)``, ``return_level_truth``, ``return_level_mean
    (P, H, W)``, ``pit (M, 10)``, ``unfitted (D,)`` and ``invalid (D,)``, the NaN cell-hours."""

    def as_dict(self, prefix: str = "extremes") -> dict:
        """flat ``{f"{prefix}/{name}/mean_extreme_bias": mean over the members, ..."_std": their population std}``, the same for
        ``return_level_bias_p{i}`` and ``return_level_rmse_p{i}``, for a logger (one device-to-host copy)"""
        if not self.variables:
            return {}
        rows, keys = [], []
        for name, v in self:
            rows.append(v["mean_extreme_bias"])
            keys.append(f"{prefix}/{name}/mean_extreme_bias")
            for i in range(int(v["periods"].shape[0])):
                for key in ("return_level_bias", "return_level_rmse"):
                    rows.append(v[key][:, i])
                    keys.append(f"{prefix}/{name}/{key}_p{i}")
        return member_mean_std(rows, keys)


def extremes_report(samples: torch.Tensor, truth: torch.Tensor, block: int, direction="max", periods: Sequence[float] = (2.0, 5.0, 10.0),
                    names: Optional[Sequence[str]] = None) -> ExtremesReport:
    """The extremes of an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` per variable: block extremes of the
    complete blocks of ``block`` hours, their L-moments, the GEV fits and the return levels of ``periods`` (in blocks).  ``names``: one
    per variable, default ``var0 ...``."""
    check_ensemble(samples, truth, time="L", members="M >= 1", floating=True)
    F = int(samples.shape[2])
    names = variable_names(names, F)
    dirn = _direction(direction, F, samples.device)
    t = block_extremes(samples, truth, block, direction)
    lmom, n_valid = lmoments(t.extremes)
    xi, alpha, k, unfitted = gev_fit(lmom)
    levels = gev_return_level(xi, alpha, k, periods)
    me_bias, me_rmse = mean_extreme_error(lmom)
    r_bias, r_rmse = lmoment_ratio_error(lmom)
    l_bias, l_rmse, l_mean = return_level_error(levels)
    regional, pit = regional_lmoments(lmom, n_valid), gev_pit(t.extremes, xi, alpha, k)
    per = torch.tensor([float(R) for R in periods], dtype=torch.float64, device=samples.device)
    variables = []
    for f in range(F):
        variables.append(dict(direction=dirn[f], periods=per, n_blocks=t.n_blocks, regional=regional[:, f], mean_extreme_bias=me_bias[:, f],
                              mean_extreme_rmse=me_rmse[:, f], ratio_bias=r_bias[:, f], ratio_rmse=r_rmse[:, f], return_level_bias=l_bias[:, f],
                              return_level_rmse=l_rmse[:, f], return_level_truth=levels[0, f], return_level_mean=l_mean[f], pit=pit[:, f],
                              unfitted=unfitted[:, f], invalid=t.invalid[:, f]))
    return ExtremesReport(names, variables)
