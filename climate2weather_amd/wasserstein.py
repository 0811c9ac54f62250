"""Ensemble sliced Wasserstein distance on the device: the distance of every member of a sampled ensemble to the truth, per variable,
and the report the reference's ``exp/metrics.py`` saves.  With ``spectra`` (MELR) and ``ssim`` this completes the three scores of
``exp/metrics.py::run``.

The reference reshapes every member to ``(time, rlat * rlon)`` on the host and calls an optimal-transport library's
``sliced_wasserstein_distance(a, b, n_projections=100, seed=0)`` in a Python loop over members (exp/metrics.py:13-44), after
normalising both arrays by the truth's moments (:254-258).  ``run_ensemble`` leaves ``(M, L, F, H, W)`` on the device, and here it
stays there: one HIP kernel (csrc/swd.hip) projects every field of the samples and of the truth onto the unit directions with an
fp32-input MFMA GEMM, a second one sorts each projected column against the truth's in LDS and writes one double.

**The definition**, in this project's words (recalled from that library's sliced distance and its 1-D distance; the library is not
available to check against -- README, "statements every number here rests on").  For one variable, samples ``X (T, d)``, truth
``Y (T, d)``, ``d = H W``, ``P`` projections, ``p = 2``:

* ``theta = numpy.random.RandomState(seed).randn(d, P)`` in float64, every column divided by its Euclidean norm -- the library's numpy
  backend's ``seed(seed); randn(d, P)``.  The same ``theta`` serves every variable, because the reference passes ``seed=0`` each time;
* ``a = X theta_p`` and ``b = Y theta_p``, column by column;
* with uniform weights and equal counts the quantile form of the 1-D distance is ``D_p = mean_i (sort(a)_i - sort(b)_i)^2``;
* ``SWD = sqrt(mean_p D_p)``;
* the reference first normalises both arrays by the truth's own moments: ``(x - gt.mean()) / gt.std()`` over all times and cells of
  the variable, the population std.

The two places that decide the definition are ``projections`` (the generator and the normalisation of its columns) and the 1-D
distance (``_general`` here, ``d_partial`` in csrc/swd_core.h).  Unequal sample and truth counts never occur in the reference (both are
selected on the observation times); they raise ``ValueError``.

**The trap.**  ``theta . ((x - mu) / sigma)`` must not be computed as ``(theta . x - mu sum(theta)) / sigma``: on a pressure field
(101 325 with a spread of 1200) that is a difference of two numbers near 1e5 in fp32.  The kernel forms ``x^ = (x - shift[f]) *
scale[f]`` in fp32 on the loaded value, before any product.

Nothing here synchronises.  A NaN in a sample field gives NaN to that (member, variable) and to no other; a NaN in a truth field gives
NaN to every member of that variable.  The reference scores DE-NORMALISED fields (``QuantileNormalizer.unnormalize`` first).

Out of scope: unequal counts and non-uniform weights, ``p != 2``, the exact ``wasserstein_distance_nd`` branch (``sliced_wd=False``
is never taken), more than 128 projections on the kernel (the general route takes them), and collectives -- members are rank-local.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, dense32, member_mean_std, variable_names
from .ensemble_host import on_device as _on_device

_THETA = {}


def projections(d: int, n_projections: int = 100, seed: int = 0, device=None) -> torch.Tensor:
    """The reference's unit directions as ``(P, d)`` fp32, K contiguous: ``RandomState(seed).randn(d, P)`` in float64 on the host, every
    column divided by its norm, rounded once.  Cached per ``(d, P, seed, device)``; the cached tensor is shared, do not write to it."""
    d, P, seed = int(d), int(n_projections), int(seed)
    if d < 1 or P < 1:
        raise ValueError("d >= 1 and n_projections >= 1")
    device = torch.device("cpu" if device is None else device)
    key = (d, P, seed, str(device))
    if key not in _THETA:
        theta = np.random.RandomState(seed).randn(d, P)
        theta = theta / np.sqrt(np.sum(theta ** 2, axis=0, keepdims=True))
        _THETA[key] = torch.from_numpy(np.ascontiguousarray(theta.T).astype(np.float32)).to(device)
    return _THETA[key]


def truth_moments(truth: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``truth (T, F, H, W)`` -> ``(shift, scale)``, each ``(F,)`` fp32 on the same device: per variable the reference's ``gt.mean()``
    and ``1 / gt.std()`` (population) over everything but F, both sums in float64, no host sync.  A constant variable has scale inf,
    as the reference divides by zero."""
    if truth.dim() != 4:
        raise ValueError(f"truth {tuple(truth.shape)} must be (T, F, H, W)")
    T, F = int(truth.shape[0]), int(truth.shape[1])
    HW = int(truth.shape[2]) * int(truth.shape[3])
    n = T * HW
    step = chunk_step(F * HW)
    mean = truth.sum(dim=(0, 2, 3), dtype=torch.float64) / n
    ss = torch.zeros(F, dtype=torch.float64, device=truth.device)
    for i in range(0, T, step):
        ss += ((truth[i:i + step].double() - mean[None, :, None, None]) ** 2).sum(dim=(0, 2, 3))
    std = torch.sqrt(ss / n)
    return mean.to(torch.float32), (1.0 / std).to(torch.float32)


def _per_variable(v, F: int, device, what: str) -> torch.Tensor:
    t = v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=torch.float64)
    t = t.to(device=device, dtype=torch.float32)
    if t.dim() > 1 or (t.dim() == 1 and t.shape[0] not in (1, F)):
        raise ValueError(f"{what}: a number or one per variable ({F})")
    return t.expand(F).contiguous()


def _general(x: torch.Tensor, y: torch.Tensor, theta: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, out: torch.Tensor) -> None:
    """The definition for any shape, any P and any device, float64 end to end: x (n_rep, T, F, d), y (T, F, d) fp32, out (n_rep, F, P)."""
    n_rep, T, F, d = x.shape
    th = theta.double().t()  # (d, P)
    s64, c64 = shift.double(), scale.double()
    for f in range(F):
        b = torch.sort(((y[:, f].double() - s64[f]) * c64[f]) @ th, dim=0).values  # the truth, projected and sorted once
        for r in range(n_rep):
            a = torch.sort(((x[r, :, f].double() - s64[f]) * c64[f]) @ th, dim=0).values
            out[r, f] = ((a - b) ** 2).mean(dim=0)


def _launch(x, y, theta, shift, scale, out, n_rep, T, F, d, P) -> bool:
    if not ops.swd_supported(d, P, T):
        return False
    px = torch.empty((n_rep, F, P, T), dtype=torch.float32, device=x.device)
    py = torch.empty((F, P, T), dtype=torch.float32, device=x.device)
    return ops.swd_project_pair(x, y, theta, shift, scale, px, py, n_rep, T, F, d, P) and ops.swd_distance(px, py, out, n_rep, F, P, T)


def sliced_wasserstein(samples: torch.Tensor, truth: torch.Tensor, *, n_projections: int = 100, seed: int = 0,
                       theta: Optional[torch.Tensor] = None, shift=None, scale=None, per_projection: bool = False) -> torch.Tensor:
    """``samples (..., T, F, H, W)`` against ``truth (T, F, H, W)`` -> the sliced Wasserstein distance of every leading index and
    variable, float64 of shape ``samples.shape[:-4] + (F,)`` on the same device (module docstring: the definition); with
    ``per_projection`` the ``D_p`` themselves, ``(..., F, P)``.  Any float dtype and any strides: a strided or 16-bit input costs one
    dense fp32 copy.  The truth is projected once and shared by all members.

    ``theta``: ``(P, d)`` unit directions, default ``projections(H W, n_projections, seed)``.  ``shift``, ``scale``: a number or one per
    variable, applied as ``(x - shift) * scale`` to both; default ``truth_moments(truth)``, the reference's normalisation;
    ``shift=0, scale=1`` scores the fields as given.

    On the GPU, ``H W`` a multiple of 64 up to 65536, ``P <= 128`` and ``T <= 16384`` take the two kernels; everything else and CPU
    tensors take the same definition in float64: the same ``x^``, ``@``, ``torch.sort``."""
    if truth.dim() != 4 or samples.dim() < 4 or tuple(samples.shape[-3:]) != tuple(truth.shape[-3:]):
        raise ValueError(f"samples {tuple(samples.shape)} must be (..., T, F, H, W) over truth {tuple(truth.shape)} = (T, F, H, W)")
    if int(samples.shape[-4]) != int(truth.shape[0]):
        raise ValueError(f"{int(samples.shape[-4])} sample times against {int(truth.shape[0])} truth times: unequal counts are not supported")
    T, F, H, W = (int(s) for s in truth.shape)
    d = H * W
    lead = tuple(samples.shape[:-4])
    x, y = dense32(samples), dense32(truth)
    if theta is None:
        theta = projections(d, n_projections, seed, x.device)
    else:
        if theta.dim() != 2 or int(theta.shape[1]) != d:
            raise ValueError(f"theta {tuple(theta.shape)} must be (P, {d})")
        theta = dense32(theta.to(x.device))
    P = int(theta.shape[0])
    if (shift is None) != (scale is None):
        raise ValueError("shift and scale: both or neither")
    if shift is None:
        shift, scale = truth_moments(y)
    else:
        shift, scale = _per_variable(shift, F, x.device, "shift"), _per_variable(scale, F, x.device, "scale")
    n_rep = math.prod(lead)
    out = torch.empty((n_rep, F, P), dtype=torch.float64, device=x.device)
    if n_rep > 0 and T > 0 and F > 0:
        x, y = x.view(n_rep, T, F, d), y.view(T, F, d)
        if not (_on_device(x) and _launch(x, y, theta, shift, scale, out, n_rep, T, F, d, P)):
            _general(x, y, theta, shift, scale, out)
    out = out.view(lead + (F, P))
    return out if per_projection else torch.sqrt(out.mean(dim=-1))


class WassersteinReport(VariableReport):
    """Per variable, what the reference's ``compute_wasserstein_nd`` returns after the normalisation of ``run`` (exp/metrics.py:254-264)
    as device tensors: ``wasserstein (M,)``; plus ``shift`` and ``scale`` (0-dim), the truth's mean and 1 / std that were applied."""

    def as_dict(self, prefix: str = "wasserstein") -> dict:
        """flat ``{name: float}`` for a logger (one device-to-host copy): per variable the mean and the standard deviation of the
        distance over the members, as the reference prints them (exp/metrics.py:291: numpy's population std)"""
        return member_mean_std([v["wasserstein"] for v in self.variables], [f"{prefix}/{name}/wasserstein" for name in self.names])


def swd_report(samples: torch.Tensor, truth: torch.Tensor, *, t_step: int = 1, n_projections: int = 100, seed: int = 0,
               names: Optional[Sequence[str]] = None) -> WassersteinReport:
    """The sliced Wasserstein distance of an ensemble ``samples (M, L, F, H, W)`` to ``truth (L, F, H, W)`` as the reference computes
    it: 100 projections from seed 0, both normalised by the truth's mean and population std per variable.  ``t_step`` keeps every
    t_step-th frame of both, as the reference restricts its scores to the observation times (exp/metrics.py:239-240) -- before the
    moments are taken, as there.  The fields are expected DE-NORMALISED, as the reference's are.  ``names``: one per variable, default
    ``var0 ...``."""
    check_ensemble(samples, truth, time="L")
    F = int(truth.shape[1])
    names = variable_names(names, F)
    t_step = int(t_step)
    if t_step < 1:
        raise ValueError("t_step >= 1")
    s, g = dense32(samples[:, ::t_step]), dense32(truth[::t_step])
    shift, scale = truth_moments(g)
    w = sliced_wasserstein(s, g, n_projections=n_projections, seed=seed, shift=shift, scale=scale)  # (M, F)
    return WassersteinReport(names, [dict(wasserstein=w[:, f], shift=shift[f], scale=scale[f]) for f in range(F)])
