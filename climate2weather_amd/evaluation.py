"""Held-out validation: the epsilon-MSE of src/thor/pipelines.py:35 on data the model was not trained on, resolved by noise level,
window frame and variable.

The reference takes ``--valid-data`` / ``--valid`` (train.py:49,68), builds the validation loader (training_loop.py:78-83,183-192) and
then prints "Validation dataset provided but currently not supported" (training_loop.py:327-330).  ``evaluate`` is that missing pass:

  * forward only -- ``Engine.forward`` without a tape, no loss fusion, nothing kept;
  * on whatever weights the network holds: what ``StandardEMA.get()`` returns, the live network, ``Trainer.validate``'s EMA copy;
  * common random numbers -- item i meets the same noise level t_i and (for a fixed batching) the same noise at every validation, so
    two checkpoints are compared on the same draws;
  * the squared error lands in a (noise-level bin x output channel) table of doubles on the device (ops.sq_err_levels: no (B,C,H,W)
    tensor, no atomics, every sum in a fixed order -- equal weights give equal bits), read back once at the end.

Why the resolution matters: the sampler's ``fold`` keeps only the CENTRE frame of a window's w = 2k + 1 output frames
(src/thor/score.py:76-88), while the training loss averages all frames, all variables and all noise levels.  ``centre_frame()`` is the
number that predicts sampling quality; ``mean()`` is the number the training loop logs.

Reproducibility: the table depends on ``(seed, n_items, batch, world)`` -- t_i on (seed, n_items), a batch's noise seed on (seed, first
item of the batch), the batch boundaries on (batch, world).  With all four fixed the result is bit-reproducible; it is NOT invariant to
the batch size or the world size (another batching draws other noise for the same item).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import ops
from .data import WindowBatch
from .ops import DTYPE_BF16, DTYPE_F16, DTYPE_F32
from .pipelines import _engine_module

_M64 = (1 << 64) - 1
_DTYPES = {"fp32": DTYPE_F32, "bf16": DTYPE_BF16, "fp16": DTYPE_F16}


def level_bins(t, bins: int) -> torch.Tensor:
    """The kernel's bin rule (include/c2w_hip.h::c2w_sq_err_levels) on the host: ``min(K - 1, floor(t * K))`` with t clamped to [0, 1]
    and ONE FP32 multiply.  In float64 the same formula gives another bin at ordinary values (K = 10: 0.7f -> 7 here, 6 in double;
    0.9f -> 9 here, 8 in double), so everything that predicts a bin goes through this function."""
    tt = torch.as_tensor(t, dtype=torch.float32).reshape(-1).clamp(0.0, 1.0)
    prod = tt * torch.tensor(float(bins), dtype=torch.float32)  # fp32 x fp32, one rounding
    return prod.floor().to(torch.int64).clamp_max(int(bins) - 1)


class LevelLoss:
    """Sums of squared errors by (noise-level bin, output channel) and the number of items per bin, both on the device.  Channel c is
    frame c // F, variable c % F of the window (dataset.py:114-126).  Every reader synchronises once; bins nothing fell into read NaN."""

    def __init__(self, bins: int, F: int, w: int, H: int, W: int, device=None):
        self.bins, self.F, self.w, self.H, self.W = int(bins), int(F), int(w), int(H), int(W)
        self.table = torch.zeros((self.bins, self.w * self.F), dtype=torch.float64, device=device)
        self.count = torch.zeros((self.bins,), dtype=torch.int64, device=device)

    @property
    def channels(self) -> int:
        return self.w * self.F

    def _host(self) -> Tuple[np.ndarray, np.ndarray]:
        """(table (K, w, F), count (K,)) as float64 arrays: ONE device-to-host copy (counts are exact in a double below 2^53)"""
        both = torch.cat((self.table.reshape(-1), self.count.to(torch.float64))).cpu().numpy()
        n = self.bins * self.channels
        return both[:n].reshape(self.bins, self.w, self.F), both[n:]

    def mean(self) -> float:
        """what ``pipeline.loss(...).mean()`` gives over the same items, noise levels and noise"""
        tab, cnt = self._host()
        return float(tab.sum() / (cnt.sum() * self.channels * self.H * self.W)) if cnt.sum() > 0 else float("nan")

    def by_level(self) -> np.ndarray:
        tab, cnt = self._host()
        with np.errstate(invalid="ignore", divide="ignore"):
            return tab.sum(axis=(1, 2)) / (cnt * self.channels * self.H * self.W)

    def by_frame(self) -> np.ndarray:
        tab, cnt = self._host()
        with np.errstate(invalid="ignore", divide="ignore"):
            return tab.sum(axis=(0, 2)) / (cnt.sum() * self.F * self.H * self.W)

    def by_variable(self) -> np.ndarray:
        tab, cnt = self._host()
        with np.errstate(invalid="ignore", divide="ignore"):
            return tab.sum(axis=(0, 1)) / (cnt.sum() * self.w * self.H * self.W)

    def centre_frame(self) -> np.ndarray:
        """(K, F): frame k = w // 2 only -- the frame the sampler's fold keeps (src/thor/score.py:76-88)"""
        tab, cnt = self._host()
        with np.errstate(invalid="ignore", divide="ignore"):
            return tab[:, self.w // 2, :] / (cnt[:, None] * self.H * self.W)

    def as_dict(self, prefix: str = "valid") -> dict:
        """flat ``{name: float}`` for a logger (one synchronisation); empty bins are left out"""
        tab, cnt = self._host()
        px, n = self.H * self.W, cnt.sum()
        out = {f"{prefix}/items": float(n)}
        if n <= 0:
            return out
        out[f"{prefix}/loss"] = float(tab.sum() / (n * self.channels * px))
        out[f"{prefix}/centre"] = float(tab[:, self.w // 2, :].sum() / (n * self.F * px))
        for i in range(self.bins):
            if cnt[i] > 0:
                out[f"{prefix}/level{i:02d}"] = float(tab[i].sum() / (cnt[i] * self.channels * px))
                out[f"{prefix}/centre_level{i:02d}"] = float(tab[i, self.w // 2].sum() / (cnt[i] * self.F * px))
        for f in range(self.w):
            out[f"{prefix}/frame{f:02d}"] = float(tab[:, f].sum() / (n * self.F * px))
        for v in range(self.F):
            out[f"{prefix}/var{v:02d}"] = float(tab[:, :, v].sum() / (n * self.w * px))
            out[f"{prefix}/centre_var{v:02d}"] = float(tab[:, self.w // 2, v].sum() / (n * px))
        return out

    def _same_shape(self, other: "LevelLoss") -> None:
        if (self.bins, self.F, self.w, self.H, self.W) != (other.bins, other.F, other.w, other.H, other.W):
            raise ValueError("LevelLoss objects of different shapes")

    def merge(self, other: "LevelLoss") -> "LevelLoss":
        self._same_shape(other)
        self.table += other.table.to(self.table.device)
        self.count += other.count.to(self.count.device)
        return self

    def all_reduce(self, group=None) -> "LevelLoss":
        """ONE sum over K * C doubles plus K counts (counts ride as doubles: exact below 2^53)"""
        import torch.distributed as dist
        buf = torch.cat((self.table.reshape(-1), self.count.to(torch.float64)))
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        n = self.bins * self.channels
        self.table.copy_(buf[:n].view_as(self.table))
        self.count.copy_(buf[n:].round().to(torch.int64))
        return self


class PlanBatch(NamedTuple):
    first: int          # global position of the batch's first item
    count: int
    t: torch.Tensor     # (count,) fp32, CPU
    noise_seed: int     # 62 bits


def _mix62(seed: int, first: int) -> int:
    """splitmix64's finaliser over (seed, first item), cut to the 62 bits the trainer's noise seeds have"""
    z = (int(seed) * 0x9E3779B97F4A7C15 + (int(first) + 1) * 0xD1B54A32D192ED03) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return (z ^ (z >> 31)) & ((1 << 62) - 1)


def validation_plan(n_items: int, batch: int, seed: int = 0, shard: Tuple[int, int] = (0, 1), t="stratified") -> List[PlanBatch]:
    """The batches of one rank, a pure host function.  Shards are contiguous (rank r owns items [r n / world, (r + 1) n / world)) and
    cut into batches of ``batch`` items, the last one shorter.
    ``t``: "stratified" -- t_i = (i + u_i) / n_items for the GLOBAL position i, u_i from a CPU generator seeded with ``seed``: every
    noise level is covered evenly however small the set is, and item i meets the same t at every validation; "uniform" -- torch.rand
    from the same generator; a tensor of n_items values -- taken as given.
    A batch's noise seed is a 62-bit mix of (seed, its first item): the result depends on (seed, n_items, batch, world), see the module
    docstring."""
    rank, world = int(shard[0]), int(shard[1])
    if n_items <= 0 or batch <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError(f"validation_plan: n_items = {n_items}, batch = {batch}, shard = {shard}")
    if isinstance(t, str):
        g = torch.Generator().manual_seed(int(seed))
        if t == "stratified":
            u = torch.rand(n_items, dtype=torch.float64, generator=g)
            tt = ((torch.arange(n_items, dtype=torch.float64) + u) / n_items).to(torch.float32)
        elif t == "uniform":
            tt = torch.rand(n_items, dtype=torch.float32, generator=g)
        else:
            raise ValueError(f"t must be 'stratified', 'uniform' or a tensor, got {t!r}")
    else:
        tt = torch.as_tensor(t).detach().reshape(-1).to(device="cpu", dtype=torch.float32)
        if tt.numel() != n_items:
            raise ValueError(f"t holds {tt.numel()} values for {n_items} items")
    lo, hi = rank * n_items // world, (rank + 1) * n_items // world
    return [PlanBatch(f, min(batch, hi - f), tt[f: min(f + batch, hi)].contiguous(), _mix62(seed, f)) for f in range(lo, hi, batch)]


class _Source:
    """items of a validation set by global position: (n, F, w, H, W, get(first, count) -> (B,C,H,W) tensor or WindowBatch)"""

    def __init__(self, data, dev, window: Optional[int]):
        self.dev = dev
        if hasattr(data, "ordered_batch"):  # DeviceWindowFeed: batches in dataset order, the feed's sampler is not consulted
            self.n = data.data.shape[0] - data.window + 1
            self.F, self.w, (self.H, self.W) = data.data.shape[1], data.window, data.data.shape[2:]
            self.get = data.ordered_batch if data.data.device == dev else _Source._windows(data.data.to(dev), data.window)
        elif hasattr(data, "data") and hasattr(data, "window"):  # a dataset with the COSMODataset item contract (dataset.py:114-126)
            self.n = data.data.shape[0] - data.window + 1
            self.F, self.w, (self.H, self.W) = data.data.shape[1], data.window, data.data.shape[2:]
            self.get = _Source._windows(data.data.to(device=dev, dtype=torch.float32).contiguous(), data.window)
        else:
            parts = [data] if isinstance(data, torch.Tensor) else list(data)
            if not parts or any(p.dim() != 4 or p.shape[1:] != parts[0].shape[1:] for p in parts):
                raise ValueError("evaluate: data must be a feed / dataset with .data and .window, a (N,C,H,W) tensor or an iterable of them")
            C, self.H, self.W = parts[0].shape[1:]
            self.w = int(window) if window else 1
            if C % self.w:
                raise ValueError(f"{C} channels are not {self.w} frames of equal width")
            self.F = C // self.w
            starts = np.cumsum([0] + [p.shape[0] for p in parts])
            self.n = int(starts[-1])

            def get(first, count):
                out, j = [], int(np.searchsorted(starts, first, side="right")) - 1
                while count > 0:
                    o = first - int(starts[j])
                    take = min(count, parts[j].shape[0] - o)
                    out.append(parts[j][o: o + take])
                    first, count, j = first + take, count - take, j + 1
                return (out[0] if len(out) == 1 else torch.cat(out)).to(dev)
            self.get = get

    @staticmethod
    def _windows(arr, window):
        return lambda first, count: WindowBatch(arr, torch.arange(first, first + count, dtype=torch.int64, device=arr.device), window)


def evaluate(net, pipeline, data, *, batch: int, bins: int = 10, seed: int = 0, precision: Optional[str] = None, shard: Tuple[int, int] = (0, 1),
             max_items: Optional[int] = None, out: Optional[LevelLoss] = None, t="stratified", eps: Optional[torch.Tensor] = None,
             window: Optional[int] = None) -> LevelLoss:
    """The validation pass over ``data`` on the weights ``net`` holds.
    ``net``: an engine-backed ScoreUNet (for instance what ``StandardEMA.get()`` returns) or a DDP / Fabric wrapper around one.
    ``data``: a DeviceWindowFeed or a dataset with ``.data`` / ``.window`` (lazy WindowBatches in dataset order; a feed's sampler state
    is not touched), a (N,C,H,W) tensor, or an iterable of (B,C,H,W) tensors (``window``: frames per item for these two; default 1).
    ``precision``: "fp32" / "bf16" / "fp16"; None: the network's own (ScoreUNet.compute_dtype).
    ``shard`` = (rank, world): this process's contiguous share; all-reduce the result (LevelLoss.all_reduce) for the whole set.
    ``t`` / ``eps`` (tests): noise levels (n_items,) and noise (n_items,C,H,W) to use instead of the plan's draws.
    Per batch: ops.mu_sigma, Engine.forward(noise=(seed, musig), nhwc_out=True) as inference, ops.sq_err_levels on the returned rows --
    on the caller's stream, without consuming any torch RNG and without touching the module's train / eval flag.  Nothing synchronises
    before the returned object is read."""
    core = _engine_module(net)
    if core is None:
        raise TypeError("evaluate needs an engine-backed ScoreUNet (or a wrapper around one)")
    eng = core._get_engine()
    dt = core.compute_dtype() if precision is None else _DTYPES[precision]
    dev, lay = eng.flat.device, eng.layout
    src = _Source(data, dev, window)
    n = src.n if max_items is None else min(src.n, int(max_items))
    C, HW = src.w * src.F, src.H * src.W
    if C != lay.out_channels:
        raise ValueError(f"items have {C} channels, the network predicts {lay.out_channels}")
    res = out if out is not None else LevelLoss(bins, src.F, src.w, src.H, src.W, device=dev)
    if (res.bins, res.F, res.w, res.H, res.W) != (int(bins), src.F, src.w, src.H, src.W):
        raise ValueError("`out` was made for another shape or number of bins")
    if eps is not None and tuple(eps.shape) != (src.n if eps.shape[0] == src.n else n, C, src.H, src.W):
        raise ValueError(f"eps must be (n_items, {C}, {src.H}, {src.W})")
    plan = validation_plan(n, batch, seed, shard, t)
    if not plan:
        return res
    t_all = torch.cat([p.t for p in plan]).to(dev)  # one upload for the whole shard
    off = 0
    with torch.no_grad():
        for p in plan:
            B = p.count
            tb = t_all[off: off + B]
            off += B
            x = src.get(p.first, B)
            musig = torch.empty((B, 2), dtype=torch.float32, device=dev)
            ops.mu_sigma(tb, musig, B, float(pipeline.eta))
            noise = p.noise_seed if eps is None else eps[p.first: p.first + B].to(device=dev, dtype=torch.float32).contiguous()
            y = eng.forward(x, tb, dt, tape=None, noise=(noise, musig), nhwc_out=True)
            scratch = eng.det_scratch(ops.sq_err_levels_scratch_bytes(B, C, HW))  # fixed-order sums whatever Engine.deterministic says
            if not ops.sq_err_levels(y, noise, tb, res.table, res.count, None, B, C, HW, lay.cout_pad, res.bins, scratch, dt):
                noise_t = torch.empty((B, C, src.H, src.W), dtype=torch.float32, device=dev)  # shape outside the regenerating kernel
                ops.philox_normal(noise_t, noise_t.numel(), noise)
                ops.sq_err_levels(y, noise_t, tb, res.table, res.count, None, B, C, HW, lay.cout_pad, res.bins, scratch, dt)
    return res
