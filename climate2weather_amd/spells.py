"""Event spells of an ensemble on the device: *how long does the event last?*  ``events.py`` asks per plane whether a value beyond a
threshold was forecast, ``temporal.py`` how much a field changes from hour to hour; neither can tell a calm of 30 hours from fifteen
calms of two.  A member that is too smooth in time makes spells too long and too few, and a sampler guided every ``t_step`` hours may
start and end them at observation times.  Spells run along time and a year of fields does not arrive at once, so the statistics are
**carried across blocks** of times: ``SpellAccumulator.update`` takes the fields block by block at bounded memory.

**The event** is that of ``events.py`` (its ``_event_spec`` and ``_indicator`` are used here): ``thresholds (F, K)`` fp32 -- a float64
threshold is rounded once -- with a direction per entry, ``"above"`` (``x >= thr``) or ``"below"`` (``x <= thr``); IEEE comparisons on
exact fp32 values, infinities compare as numbers, a NaN is no event.

**Rows.**  ``d = 0`` is the truth if one is given, then the ``M`` members: ``D = M + 1``, or ``M`` without a truth.

**Series and spells.**  One series exists per ``(d, f, k, cell)``: the indicator ``e[t]`` over all times seen so far.  A spell is a
maximal run of consecutive 1s, its length ``L`` the hours in it.  A NaN ends a spell like any non-event; NaN cell-hours are counted
apart per ``(d, f)`` in ``invalid``.  A run that touches the first or the last time seen is a spell of its observed length: censored
spells are **counted, not dropped** -- a stated choice -- and ``censored`` says how many there were.

**The tables** (include/c2w_hip.h: c2w_spell_update), every integer exact:

* ``hist[d, f, k, b]``, int64 ``(D, F, K, Lmax)``: the spells of all cells with ``L = b + 1``; the last bin holds ``L >= Lmax``
  (``Lmax = max_duration``, default 48).
* ``hours``, ``count``, ``longest``, int32 ``(D, F, K, H, W)``: event hours, number of spells and longest spell of each cell's series
  -- the climate-index maps (frost hours, number of heat spells, longest calm).
* ``onsets[d, f, k, phi]``, int64 ``(D, F, K, period)``: the spells whose first hour ``t`` has ``(t0 + t) mod period = phi``, ``t``
  counted from the first block.  A run already open at the very first time is an onset there; ``period = 0`` builds none.
* ``invalid[d, f]``, int64: NaN cell-hours.  ``censored[d, f, k]``, int64: the spells that touch the first or the last time seen.

**The state.**  ``state (4, D, F, K, H W)`` int32 holds per series ``open`` (the length of the run open at the last time seen), and
``longest``, ``count``, ``hours``; an update reads it at the start and writes it at the end and adds the spells that ENDED to ``hist``
and the onsets to ``onsets``.  ``tables()`` closes the open runs on a copy with a handful of torch operations -- the bins of
``min(open, Lmax)``, ``count + (open > 0)``, ``max(longest, open)`` -- and leaves the state alone, so updating may go on.  The total
time stays under ``2^31``.

**The scores** are float64 algebra on the tables, any leading shape: ``duration_pmf``, ``survival`` (``P(L >= l)``),
``mean_duration = sum hours / sum count`` (exact even when the last bin is populated), ``event_frequency``,
``spell_duration_distance`` (the 1-Wasserstein distance between the duration PMFs of a member and of the truth,
``sum_{l < Lmax} |P(L <= l) - Q(L <= l)|`` -- a LOWER BOUND once the last bin is populated, since lengths beyond ``Lmax`` are told
apart no more), ``longest_spell_error`` (bias and RMSE of a member's ``longest`` map against the truth's), ``onset_share`` and
``spells_report``.

On the GPU ``H W`` a multiple of 4, ``K <= 8``, ``max_duration <= 256`` and ``period <= 24`` take the kernel (csrc/spells.hip), which
splits rows, variables and cells over the workgroups but never one block's time axis.  Everything else and CPU tensors take the same
integers from torch, vectorised over time with a running maximum.  Nothing here synchronises.

Out of scope: spells joint over variables or over neighbouring cells, minimum-gap merging of spells, the time-segmented kernel,
extreme-value fits, collectives -- members are rank-local -- and the plotting.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import spell_ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, datasets, member_mean_std, variable_names
from .ensemble_host import on_device as _on_device
from .events import _event_spec, _indicator

MAX_TIME = (1 << 31) - 1   # the counters of the state are int32
MAX_BLOCK = 1 << 20        # times one launch takes (csrc/spells_core.h: MAX_T); a longer block is walked in parts
OPEN, LONGEST, COUNT, HOURS = 0, 1, 2, 3


class SpellTables(NamedTuple):
    """What ``SpellAccumulator.tables`` returns, the open runs closed (module docstring)"""
    hist: torch.Tensor      # (D, F, K, Lmax) int64
    hours: torch.Tensor     # (D, F, K, H, W) int32
    count: torch.Tensor     # (D, F, K, H, W) int32
    longest: torch.Tensor   # (D, F, K, H, W) int32
    onsets: torch.Tensor    # (D, F, K, period) int64
    invalid: torch.Tensor   # (D, F) int64
    censored: torch.Tensor  # (D, F, K) int64
    n_times: int


# ---------------------------------------------------------------------------------------------------------------------- one block

def _general(x, y, thr, dirn, state, hist, onsets, invalid, max_duration: int, period: int, t_abs: int) -> None:
    """The definition for any shape and any device, vectorised over time: with ``lastzero[t]`` the last time ``<= t`` without the
    event (-1: none in this block) a run that ends at ``t`` has length ``t - lastzero[t]``, plus the carried ``open`` where
    ``lastzero[t] = -1``.  x (M, T, F, hw), y (T, F, hw) or None; the rest as ``spell_ops.spell_update`` takes it."""
    M, T, F, hw = (int(s) for s in x.shape)
    D, K = int(state.shape[1]), int(thr.shape[1])
    th, dr = thr[:, :, None], dirn[:, :, None]
    row = torch.arange(D * F * K, device=x.device).view(1, D, F, K, 1)
    step = chunk_step(D * F * K * hw * 8)
    for s0 in range(0, T, step):
        rows = x[:, s0:s0 + step] if y is None else torch.cat([y[None, s0:s0 + step], x[:, s0:s0 + step]])   # (D, n, F, hw)
        n = int(rows.shape[1])
        invalid += torch.isnan(rows).sum(dim=(1, 3))
        e = _indicator(rows[:, :, :, None, :], th, dr).permute(1, 0, 2, 3, 4)                                # (n, D, F, K, hw) bool
        open_in = state[OPEN].to(torch.int64)
        tt = torch.arange(n, device=x.device).view(n, 1, 1, 1, 1)
        lastzero = torch.where(e, torch.full_like(tt, -1), tt).cummax(dim=0).values
        length = tt - lastzero + torch.where(lastzero < 0, open_in, torch.zeros_like(open_in))               # of the run that holds t
        was_open = open_in > 0
        ends = e & ~torch.cat([e[1:], torch.ones_like(e[:1])])       # the block's end closes nothing
        starts = e & ~torch.cat([was_open[None], e[:-1]])            # a run carried in does not begin here
        # the spells that end in this block: those above and the carried run the first plane ends
        ended = torch.cat([ends, (~e[0] & was_open)[None]])
        L = torch.where(ended, torch.cat([length, open_in[None]]), torch.zeros_like(ended, dtype=torch.int64))
        hist.view(-1).scatter_add_(0, (row * max_duration + L.clamp(1, max_duration) - 1).reshape(-1), ended.to(torch.int64).reshape(-1))
        if period:
            phase = (t_abs + s0 + tt) % period
            onsets.view(-1).scatter_add_(0, (row * period + phase).expand(starts.shape).reshape(-1), starts.to(torch.int64).reshape(-1))
        state[COUNT] += ended.sum(dim=0).to(torch.int32)
        state[LONGEST] = torch.maximum(state[LONGEST], L.max(dim=0).values.to(torch.int32))
        state[HOURS] += e.sum(dim=0).to(torch.int32)
        state[OPEN] = torch.where(e[-1], length[-1], torch.zeros_like(open_in)).to(torch.int32)


def _launch(x, y, thr, dirn, state, hist, onsets, invalid, max_duration: int, period: int, t_abs: int) -> bool:
    M, T, F, hw = (int(s) for s in x.shape)
    K = int(thr.shape[1])
    if not spell_ops.supported(hw, K, max_duration, period):
        return False
    return spell_ops.spell_update(x, y, thr, dirn, state, hist, onsets if period else None, invalid, M, T, F, hw, K, max_duration, period, t_abs)


# ---------------------------------------------------------------------------------------------------------------------- the accumulator

def _count(value, name: str, low: int) -> int:
    if isinstance(value, bool) or int(value) != value or int(value) < low:
        raise ValueError(f"{name} {value!r} must be an integer >= {low}")
    return int(value)


class SpellAccumulator:
    """Spell statistics of ``M`` members (and the truth) of ``F`` variables on ``H x W`` cells, carried from block to block:

        acc = SpellAccumulator(M, F, H, W, thresholds, "below", period=6, device=samples.device)
        for samples, truth in blocks:          # (M, T, F, H, W), (T, F, H, W); any T >= 0
            acc.update(samples, truth)
        tables = acc.tables()

    ``thresholds (F, K)`` and ``direction`` as in ``events.event_counts``.  ``with_truth=False``: the rows are the members alone and
    ``update`` takes no truth.  ``max_duration``: the bins of ``hist``; ``period``: the phases of ``onsets`` (0: none); ``t0``: the
    absolute hour of the first plane of the first block.  The memory is that of the state, ``16 D F K H W`` bytes, whatever the length
    of the run."""

    def __init__(self, M: int, F: int, H: int, W: int, thresholds, direction="above", *, with_truth: bool = True, max_duration: int = 48,
                 period: int = 0, t0: int = 0, device=None):
        self.M, self.F, self.H, self.W = _count(M, "M", 1), _count(F, "F", 1), _count(H, "H", 1), _count(W, "W", 1)
        self.max_duration, self.period, self.t0 = _count(max_duration, "max_duration", 1), _count(period, "period", 0), _count(t0, "t0", 0)
        self.with_truth = bool(with_truth)
        self.device = torch.device("cpu" if device is None else device)
        self.thr, self.dirn = _event_spec(thresholds, direction, self.F, self.device)
        self.D, self.K = self.M + (1 if self.with_truth else 0), int(self.thr.shape[1])
        D, K, hw = self.D, self.K, self.H * self.W
        self.state = torch.zeros((4, D, self.F, K, hw), dtype=torch.int32, device=self.device)
        self.hist = torch.zeros((D, self.F, K, self.max_duration), dtype=torch.int64, device=self.device)
        self.onsets = torch.zeros((D, self.F, K, self.period), dtype=torch.int64, device=self.device)
        self.invalid = torch.zeros((D, self.F), dtype=torch.int64, device=self.device)
        self.first = torch.zeros((D, self.F, K), dtype=torch.int64, device=self.device)  # the series with the event at the very first time
        self.n_times = 0

    def update(self, samples: torch.Tensor, truth: Optional[torch.Tensor] = None) -> "SpellAccumulator":
        """``samples (M, T, F, H, W)`` and, with a truth, ``truth (T, F, H, W)``: the next ``T >= 0`` times.  Any float dtype and any
        strides: a strided or 16-bit input costs one dense fp32 copy of the block."""
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
            raise ValueError(f"the block must be on {self.device}, the accumulator's device")
        T = int(samples.shape[1])
        if self.n_times + T > MAX_TIME:
            raise ValueError(f"{self.n_times} + {T} times: the total time must stay under 2^31")
        for s in range(0, T, MAX_BLOCK):
            self._block(samples[:, s:s + MAX_BLOCK], None if truth is None else truth[s:s + MAX_BLOCK])
        return self

    def _block(self, samples, truth) -> None:
        x, y, _ = datasets(samples, truth)
        T = int(x.shape[1])
        if self.n_times == 0:
            rows = x[:, 0] if y is None else torch.cat([y[None, 0], x[:, 0]])                                 # (D, F, hw)
            self.first = _indicator(rows[:, :, None, :], self.thr[:, :, None], self.dirn[:, :, None]).sum(dim=-1)
        args = (x, y, self.thr, self.dirn, self.state, self.hist, self.onsets, self.invalid, self.max_duration, self.period,
                self.t0 + self.n_times)
        if not (_on_device(x) and _launch(*args)):
            _general(*args)
        self.n_times += T

    def tables(self) -> SpellTables:
        """The tables with the open runs closed; the state is left alone"""
        D, F, K, Lmax = self.D, self.F, self.K, self.max_duration
        open_, longest, count, hours = self.state.unbind(0)
        is_open = open_ > 0
        row = torch.arange(D * F * K, device=self.device).view(D, F, K, 1)
        hist = self.hist.clone()
        hist.view(-1).scatter_add_(0, (row * Lmax + open_.to(torch.int64).clamp(1, Lmax) - 1).reshape(-1), is_open.to(torch.int64).reshape(-1))
        whole = is_open & (open_ == self.n_times)  # open since the very first time: it touches both ends and is one spell
        censored = self.first + is_open.sum(dim=-1) - whole.sum(dim=-1)
        shape = (D, F, K, self.H, self.W)
        return SpellTables(hist, hours.clone().view(shape), (count + is_open.to(torch.int32)).view(shape),
                           torch.maximum(longest, open_).view(shape), self.onsets.clone(), self.invalid.clone(), censored, self.n_times)

    def state_dict(self) -> dict:
        """everything a later ``load_state_dict`` needs to go on where this run stopped (copies)"""
        return dict(state=self.state.clone(), hist=self.hist.clone(), onsets=self.onsets.clone(), invalid=self.invalid.clone(),
                    first=self.first.clone(), n_times=self.n_times, t0=self.t0, max_duration=self.max_duration, period=self.period,
                    thresholds=self.thr.clone(), direction=self.dirn.clone())

    def load_state_dict(self, sd: dict) -> "SpellAccumulator":
        for key in ("t0", "max_duration", "period"):
            if int(sd[key]) != getattr(self, key):
                raise ValueError(f"{key} {sd[key]} of the state differs from this accumulator's {getattr(self, key)}")
        if not (torch.equal(sd["thresholds"].to(self.device), self.thr) and torch.equal(sd["direction"].to(self.device), self.dirn)):
            raise ValueError("the thresholds or directions of the state differ from this accumulator's")
        for key in ("state", "hist", "onsets", "invalid", "first"):
            mine = getattr(self, key)
            if tuple(sd[key].shape) != tuple(mine.shape):
                raise ValueError(f"{key} {tuple(sd[key].shape)} of the state must be {tuple(mine.shape)}")
        for key in ("state", "hist", "onsets", "invalid", "first"):
            setattr(self, key, sd[key].to(device=self.device, dtype=getattr(self, key).dtype).clone().contiguous())
        self.n_times = int(sd["n_times"])
        return self


def spell_tables(samples: torch.Tensor, truth: Optional[torch.Tensor], thresholds, direction="above", max_duration: int = 48, period: int = 0,
                 t0: int = 0) -> SpellTables:
    """One update plus ``tables()``: ``samples (M, T, F, H, W)``, ``truth (T, F, H, W)`` or None"""
    if samples.dim() != 5:
        raise ValueError(f"samples {tuple(samples.shape)} must be (M, T, F, H, W)")
    M, _, F, H, W = (int(s) for s in samples.shape)
    acc = SpellAccumulator(M, F, H, W, thresholds, direction, with_truth=truth is not None, max_duration=max_duration, period=period, t0=t0,
                           device=samples.device)
    return acc.update(samples, truth).tables()


# ---------------------------------------------------------------------------------------------------------------------- the algebra

def _hist(hist: torch.Tensor) -> torch.Tensor:
    if hist.dim() < 1 or int(hist.shape[-1]) < 1:
        raise ValueError(f"hist {tuple(hist.shape)} must be (..., Lmax)")
    return hist.to(torch.float64)


def duration_pmf(hist: torch.Tensor) -> torch.Tensor:
    """``hist (..., Lmax)`` -> float64 of the same shape: the share of the spells with ``L = b + 1`` (last bin: ``L >= Lmax``); NaN
    without a spell"""
    h = _hist(hist)
    return h / h.sum(dim=-1, keepdim=True)


def survival(hist: torch.Tensor) -> torch.Tensor:
    """``P(L >= l)`` for ``l = 1 .. Lmax``, float64 ``(..., Lmax)``; exact in every entry, the last bin being ``L >= Lmax``"""
    h = _hist(hist)
    return h.flip(-1).cumsum(dim=-1).flip(-1) / h.sum(dim=-1, keepdim=True)  # the running sums are of integers: exact in any order


def _number(n: int, like: torch.Tensor) -> torch.Tensor:
    """``n`` as a float64 tensor next to ``like``: a quotient of two tensors is a division on every device, where one by a Python
    number may become a product with the reciprocal"""
    return torch.full((), float(n), dtype=torch.float64, device=like.device)


def _maps(a: torch.Tensor, name: str) -> torch.Tensor:
    if a.dim() < 2:
        raise ValueError(f"{name} {tuple(a.shape)} must be (..., H, W)")
    return a.to(torch.float64)


def mean_duration(hours: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """``hours, count (..., H, W)`` -> ``(...)`` float64: ``sum hours / sum count`` over the cells, exact even when the last bin of
    ``hist`` is populated; NaN without a spell"""
    if tuple(hours.shape) != tuple(count.shape):
        raise ValueError(f"hours {tuple(hours.shape)} and count {tuple(count.shape)} must have one shape")
    return _maps(hours, "hours").sum(dim=(-1, -2)) / _maps(count, "count").sum(dim=(-1, -2))


def event_frequency(hours: torch.Tensor, n_times: int) -> torch.Tensor:
    """``hours (..., H, W)`` -> ``(...)`` float64: the share of the cell-hours with the event"""
    h = _maps(hours, "hours")
    return h.sum(dim=(-1, -2)) / _number(int(h.shape[-1]) * int(h.shape[-2]) * int(n_times), h)


def spell_duration_distance(hist: torch.Tensor) -> torch.Tensor:
    """``hist (..., D, F, K, Lmax)`` with row 0 the truth -> ``(..., D - 1, F, K)`` float64: the 1-Wasserstein distance between the
    duration PMFs of each member and of the truth, ``sum_{l < Lmax} |P(L <= l) - Q(L <= l)|``, in hours.  Lengths of ``Lmax`` and
    beyond share the last bin, so this is a LOWER BOUND of the distance once that bin is populated.  NaN where either has no spell."""
    if hist.dim() < 4 or int(hist.shape[-4]) < 2:
        raise ValueError(f"hist {tuple(hist.shape)} must be (..., D >= 2, F, K, Lmax), row 0 the truth")
    h = _hist(hist)
    cdf = h.cumsum(dim=-1)[..., :-1] / h.sum(dim=-1, keepdim=True)  # integers first, one division: the same bits on every device
    return (cdf[..., 1:, :, :, :] - cdf[..., :1, :, :, :]).abs().sum(dim=-1)


def longest_spell_error(longest: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``longest (..., D, F, K, H, W)`` with row 0 the truth -> ``(bias, rmse)``, each ``(..., D - 1, F, K)`` float64, of each member's
    map of the longest spell against the truth's, over the cells"""
    if longest.dim() < 5 or int(longest.shape[-5]) < 2:
        raise ValueError(f"longest {tuple(longest.shape)} must be (..., D >= 2, F, K, H, W), row 0 the truth")
    m = _maps(longest, "longest")
    diff = m[..., 1:, :, :, :, :] - m[..., :1, :, :, :, :]
    cells = _number(int(m.shape[-1]) * int(m.shape[-2]), m)
    return diff.sum(dim=(-1, -2)) / cells, ((diff * diff).sum(dim=(-1, -2)) / cells).sqrt()


def onset_share(onsets: torch.Tensor) -> torch.Tensor:
    """``onsets (..., period)`` -> float64 of the same shape: the share of the onsets at each phase; NaN without a spell"""
    if onsets.dim() < 1 or int(onsets.shape[-1]) < 1:
        raise ValueError(f"onsets {tuple(onsets.shape)} must be (..., period >= 1)")
    o = onsets.to(torch.float64)
    return o / o.sum(dim=-1, keepdim=True)


# ---------------------------------------------------------------------------------------------------------------------- the report

class SpellsReport(VariableReport):
    """Per variable, as device tensors, ``K`` thresholds, ``D`` rows (0 the truth): ``thresholds (K,)``, ``event_frequency``,
    ``mean_duration``, ``spells``, ``censored``, ``longest_max (D, K)``, ``duration_pmf``, ``survival (D, K, Lmax)``,
    ``duration_distance``, ``longest_bias``, ``longest_rmse (M, K)``, ``onset_share (D, K, period)`` where ``period > 0``, and
    ``invalid (D,)``, the NaN cell-hours."""

    def as_dict(self, prefix: str = "spells") -> dict:
        """flat ``{f"{prefix}/{name}/mean_duration_k{k}": mean over the members, ..."_std": their population std}``, the same for
        ``duration_distance`` and ``longest_bias``, for a logger (one device-to-host copy)"""
        if not self.variables:
            return {}
        rows, keys = [], []
        for name, v in self:
            for k in range(int(v["thresholds"].shape[0])):
                for key, t in (("mean_duration", v["mean_duration"][1:, k]), ("duration_distance", v["duration_distance"][:, k]),
                               ("longest_bias", v["longest_bias"][:, k])):
                    rows.append(t)
                    keys.append(f"{prefix}/{name}/{key}_k{k}")
        return member_mean_std(rows, keys)


def spells_report(samples: torch.Tensor, truth: torch.Tensor, thresholds, direction="above", max_duration: int = 48, period: int = 0,
                  t0: int = 0, names: Optional[Sequence[str]] = None) -> SpellsReport:
    """The spell statistics of an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` per variable, from one pass over
    the fields.  ``names``: one per variable, default ``var0 ...``."""
    check_ensemble(samples, truth, time="L", members="M >= 1", floating=True)
    F = int(samples.shape[2])
    names = variable_names(names, F)
    thr, _ = _event_spec(thresholds, direction, F, samples.device)
    t = spell_tables(samples, truth, thr, direction, max_duration, period, t0)
    freq, mean = event_frequency(t.hours, t.n_times), mean_duration(t.hours, t.count)
    pmf, surv, dist = duration_pmf(t.hist), survival(t.hist), spell_duration_distance(t.hist)
    bias, rmse = longest_spell_error(t.longest)
    spells, top = t.count.sum(dim=(-1, -2), dtype=torch.int64), t.longest.amax(dim=(-1, -2))
    share = onset_share(t.onsets) if period else None
    variables = []
    for f in range(F):
        v = dict(thresholds=thr[f], event_frequency=freq[:, f], mean_duration=mean[:, f], spells=spells[:, f], censored=t.censored[:, f],
                 longest_max=top[:, f], duration_pmf=pmf[:, f], survival=surv[:, f], duration_distance=dist[:, f], longest_bias=bias[:, f],
                 longest_rmse=rmse[:, f], invalid=t.invalid[:, f])
        if share is not None:
            v["onset_share"] = share[:, f]
        variables.append(v)
    return SpellsReport(names, variables)
