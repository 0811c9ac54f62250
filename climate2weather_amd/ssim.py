"""Ensemble SSIM on the device: the mean structural similarity of every member and frame of a sampled ensemble to the truth, and the
per-variable report the reference's ``exp/metrics.py`` saves.

The reference loops in Python over every member and time of a netCDF array on the host and calls an image library's
``structural_similarity(win_size=15)`` on each pair (exp/metrics.py:187-212), a few milliseconds a call; ``run_ensemble`` leaves
``(M, L, F, H, W)`` on the device, and here it stays there: one HIP kernel (csrc/ssim.hip) reads each sample field once, the truth with
it, and writes one double per pair.

**The definition**, in this project's words (recalled from that library's ``structural_similarity`` with its defaults, Gaussian
weighting off as the reference leaves it; the library is not available to check against -- README, "statements every number here
rests on").  For a pair ``x``, ``y`` of ``H x W``, window ``w`` odd, ``NP = w^2``, ``cn = NP / (NP - 1)`` (sample covariance), data
range ``R``:

* ``u_a`` is the mean of ``a`` over the ``w x w`` window, for ``a`` in ``x, y, xx, yy, xy``;
* ``vx = cn (u_xx - u_x^2)``, ``vy`` likewise, ``vxy = cn (u_xy - u_x u_y)``;
* ``C1 = (0.01 R)^2``, ``C2 = (0.03 R)^2``;
* ``S = (2 u_x u_y + C1)(2 vxy + C2) / ((u_x^2 + u_y^2 + C1)(vx + vy + C2))``;
* the score is the mean of ``S`` over the ``(H - w + 1)(W - w + 1)`` windows that lie fully inside the field -- the library's crop by
  ``(w - 1) / 2``, so its border mode never matters;
* ``R`` is the reference's: ``max(truth.max, samples.max) - min(truth.min, samples.min)`` over ALL times and members of one variable
  (exp/metrics.py:194-196).

**The trap.**  De-normalised fields carry offsets (a pressure near 101 325 with a spread of 1200), and ``u_xx - u_x^2`` in fp32 on such
a field is a difference of two numbers near 1e10: a straight fp32 port is off by 1e-3 in the score.  The kernel takes one pivot -- the
truth field's mean, from a double sum -- off both fields before any product.  Variances and the covariance are shift invariant; only
the luminance factor needs the pivot back, and it is formed as ``1 - (u_x - u_y)^2 / (u_x^2 + u_y^2 + C1)``.

Nothing here synchronises.  A NaN in a pair gives that pair NaN and no other -- unless the data range is left to be computed, which
then is NaN for the whole variable, as the reference's is.  The reference scores DE-NORMALISED fields
(``QuantileNormalizer.unnormalize`` first, exp/exputil.py): do the same before calling this.

Out of scope: Gaussian weighting, the SSIM map itself, a tiled kernel for the deep variant's 256 x 256 (the general route takes it),
and collectives -- members are rank-local, gathering a report across ranks is the caller's.  The sliced-Wasserstein score of
exp/metrics.py is in ``climate2weather_amd.wasserstein``.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .ensemble_host import VariableReport, check_ensemble, dense32, member_mean_std, variable_names
from .ensemble_host import on_device as _on_device

POOL_CHUNK_ELEMS = 1 << 21  # values of one field stack per general-route chunk (16 MiB of float64, about ten such stacks alive)


def global_range(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The reference's data range, per variable, on the device and without a host sync: ``x (n_rep, *lead, H, W)`` samples against
    ``y (*lead, H, W)`` truth -> ``lead``-shaped fp32.  With two or more leading dimensions the last of them is the variable (truth
    ``(T, F, H, W)``): each variable gets ``max - min`` over everything else of both tensors.  With fewer -- ``(H, W)`` or
    ``(T, H, W)`` -- the whole of both tensors is one variable."""
    lead = tuple(y.shape[:-2])
    if len(lead) >= 2:
        F = lead[-1]
        xs, ys = x.reshape(-1, F, x.shape[-2] * x.shape[-1]), y.reshape(-1, F, y.shape[-2] * y.shape[-1])
        hi = torch.maximum(xs.amax(dim=(0, 2)), ys.amax(dim=(0, 2)))
        lo = torch.minimum(xs.amin(dim=(0, 2)), ys.amin(dim=(0, 2)))
    else:
        hi, lo = torch.maximum(x.amax(), y.amax()), torch.minimum(x.amin(), y.amin())
    return (hi - lo).to(torch.float32).expand(lead)


def _ssim_general(x: torch.Tensor, y: torch.Tensor, rng: torch.Tensor, out: torch.Tensor, win: int) -> None:
    """The definition for any (H, W), any odd window and any device: float64 ``avg_pool2d`` in chunks of bounded size.  In float64 the
    straight form needs no pivot (a pressure field loses 1e-12 of its variance to it)."""
    n, H, W = x.shape
    nt = y.shape[0]
    NP = win * win
    cn = NP / (NP - 1.0)
    step = max(1, POOL_CHUNK_ELEMS // (H * W))

    def pool(t):
        return torch.nn.functional.avg_pool2d(t[:, None], win, stride=1)[:, 0]

    for i in range(0, n, step):
        idx = torch.arange(i, min(n, i + step), device=x.device) % nt
        a, b = x[i:i + step].double(), y.index_select(0, idx).double()
        R = rng.index_select(0, idx).double()[:, None, None]
        C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        ua, ub = pool(a), pool(b)
        va, vb, vab = cn * (pool(a * a) - ua * ua), cn * (pool(b * b) - ub * ub), cn * (pool(a * b) - ua * ub)
        S = ((2.0 * ua * ub + C1) * (2.0 * vab + C2)) / ((ua * ua + ub * ub + C1) * (va + vb + C2))
        out[i:i + step] = S.mean(dim=(-2, -1))


def ssim(samples: torch.Tensor, truth: torch.Tensor, *, data_range=None, win_size: int = 15) -> torch.Tensor:
    """``samples (..., H, W)`` against ``truth``, whose shape is the trailing part of ``samples``' -- ``(M, T, F, H, W)`` against
    ``(T, F, H, W)`` is the documented case; flattened, pair ``i`` is ``(samples[i], truth[i % n_truth])`` -> the mean SSIM of every
    pair, float64 of shape ``samples.shape[:-2]`` on the same device (module docstring: the definition).  Any float dtype and any
    strides: a strided or 16-bit input costs one dense fp32 copy.

    ``data_range``: None computes the reference's global range per variable on the device (``global_range``); a float serves every
    pair; a tensor is broadcast to ``truth.shape[:-2]``, one range per truth slot.  ``win_size`` is odd, at least 3 and at most
    ``min(H, W)``: 15 is the reference's, 7 the library's default.

    On the GPU, H and W multiples of 8 from 16 to 128 with a window of 7, 11 or 15 take the fused kernel; every other shape -- odd,
    larger (the deep variant's 256 x 256) -- every other window and CPU tensors take the same definition through float64
    ``avg_pool2d``."""
    if samples.dim() < 2 or truth.dim() < 2 or truth.dim() > samples.dim() or tuple(samples.shape[samples.dim() - truth.dim():]) != tuple(truth.shape):
        raise ValueError(f"truth {tuple(truth.shape)} must be the trailing part of samples {tuple(samples.shape)} = (..., H, W)")
    H, W = int(truth.shape[-2]), int(truth.shape[-1])
    win = int(win_size)
    if win != win_size or win < 3 or win % 2 == 0 or win > min(H, W):
        raise ValueError(f"win_size {win_size!r}: an odd number from 3 to min(H, W) = {min(H, W)}")
    lead, tlead = tuple(samples.shape[:-2]), tuple(truth.shape[:-2])
    x, y = dense32(samples), dense32(truth)
    out = torch.empty(lead, dtype=torch.float64, device=x.device)
    n, nt = out.numel(), 1
    for d in tlead:
        nt *= int(d)
    if n == 0:
        return out
    if data_range is None:
        rng = global_range(x, y)
    elif isinstance(data_range, torch.Tensor):
        rng = data_range.to(device=x.device, dtype=torch.float32).expand(tlead)
    else:
        rng = torch.full((), float(data_range), dtype=torch.float32, device=x.device).expand(tlead)
    rng = rng.reshape(nt).contiguous()
    x, y = x.view(n, H, W), y.view(nt, H, W)
    if not (_on_device(x) and ops.ssim(x, y, rng, out, n, nt, H, W, win)):
        _ssim_general(x, y, rng, out.view(n), win)
    return out


class SsimReport(VariableReport):
    """Per variable, what the reference's ``ssim()`` computes (exp/metrics.py:198-212) as device tensors: ``ssim_over_time (M, T)``,
    its ``ssim_values``, and ``ssim (M,)``, their mean over time, which is what it returns; plus ``data_range`` (0-dim), the range used."""

    def as_dict(self, prefix: str = "ssim") -> dict:
        """flat ``{name: float}`` for a logger (one device-to-host copy): per variable the mean and the standard deviation of the score
        over the members, as the reference prints them (exp/metrics.py:291: numpy's population std)"""
        return member_mean_std([v["ssim"] for v in self.variables], [f"{prefix}/{name}/ssim" for name in self.names])


def ssim_report(samples: torch.Tensor, truth: torch.Tensor, *, t_step: int = 1, win_size: int = 15,
                names: Optional[Sequence[str]] = None) -> SsimReport:
    """SSIM of an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` as the reference computes it: window 15, the data
    range of each variable taken over all kept frames and members.  ``t_step`` keeps every t_step-th frame of both, as the reference
    restricts its scores to the observation times (exp/metrics.py:239-240) -- before the range is taken, as there.  The fields are
    expected DE-NORMALISED, as the reference's are (``QuantileNormalizer.unnormalize`` first): the range and the two constants are in
    the variable's own units.  ``names``: one per variable, default ``var0 ...``."""
    check_ensemble(samples, truth, time="L")
    F = int(truth.shape[1])
    names = variable_names(names, F)
    t_step = int(t_step)
    if t_step < 1:
        raise ValueError("t_step >= 1")
    s, g = dense32(samples[:, ::t_step]), dense32(truth[::t_step])
    rng = global_range(s, g)                                   # (T, F), the same along T
    over_time = ssim(s, g, data_range=rng, win_size=win_size)  # (M, T, F)
    mean = over_time.mean(dim=1)                               # (M, F)
    return SsimReport(names, [dict(ssim_over_time=over_time[:, :, f], ssim=mean[:, f], data_range=rng[0, f]) for f in range(F)])
