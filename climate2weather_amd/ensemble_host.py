"""The host side the ensemble metrics share (``crps``, ``ssim``, ``spectra``, ``wasserstein``, ``marginals``, ``quantiles``,
``windpower``, ``multivariate``, ``temporal``, ``biascorrect``, ``events``, ``spells``, ``objects``, ``extremes``, ``dependence``, ``scalesplit``): how an input becomes what the kernels read, how the float64 routes are chunked, how scratch is
allocated, what the argument checks say and what a per-variable report is.  Plain functions; no metric imports another metric for any of
it.

**The seam.**  Which route a call takes is decided in the metric module, never here: each module binds ``on_device`` under a private
name of its own and keeps its own ``if not (<that name>(x) and _launch(...)): _general(...)`` ("Ensemble host layer").  The
emulations of the CPU tests replace that one module's name together with that module's launchers, and a metric that calls another
(``windpower`` -> ``marginals``) must find the other's route untouched.  So nothing in this file calls ``on_device``.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

CHUNK_ELEMS = 1 << 22  # values per chunk of the float64 passes (32 MiB of float64 alive at a time)


def on_device(x: torch.Tensor) -> bool:
    return x.is_cuda


def dense32(t: torch.Tensor) -> torch.Tensor:
    """``t`` as the kernels read it -- fp32, contiguous, 16-byte aligned: ``t`` itself where it already is, else one copy"""
    x = t
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = torch.empty(t.shape, dtype=torch.float32, device=t.device).copy_(t)  # the one copy: dense and fp32 at once
    if x.data_ptr() % 16 != 0:
        x = x.clone()
    return x


def chunk_step(per_item: int) -> int:
    """how many items of ``per_item`` values each a float64 pass takes at a time: ``CHUNK_ELEMS`` values, at least one item"""
    return max(1, CHUNK_ELEMS // max(1, per_item))


def scratch(nbytes: int, device, dtype: torch.dtype = torch.float64, optional: bool = True) -> Optional[torch.Tensor]:
    """``nbytes`` (what a ``*_scratch_bytes`` query said) of ``dtype`` on ``device``.  ``optional``: None where the library needs none;
    otherwise at least one element, for the entry points that want a valid pointer."""
    n = nbytes // dtype.itemsize
    if optional:
        return torch.empty((n,), dtype=dtype, device=device) if nbytes else None
    return torch.empty((max(1, n),), dtype=dtype, device=device)


def check_ensemble(samples: torch.Tensor, truth: torch.Tensor, *, time: str = "T", members: str = "M", floating: bool = False) -> None:
    """``samples (M, T, F, H, W)`` against ``truth (T, F, H, W)``.  ``time``: the letter the message gives the time axis (``"L"`` in the
    reports); ``members="M >= 1"`` also demands a member; ``floating`` also demands floating-point dtypes."""
    bad = samples.dim() != 5 or truth.dim() != 4 or tuple(samples.shape[1:]) != tuple(truth.shape)
    if bad or (members != "M" and int(samples.shape[0]) < 1):
        raise ValueError(f"samples {tuple(samples.shape)} must be ({members},) + truth {tuple(truth.shape)} = ({time}, F, H, W)")
    if floating and not (samples.is_floating_point() and truth.is_floating_point()):
        raise ValueError(f"samples ({samples.dtype}) and truth ({truth.dtype}) must be floating point")


def variable_names(names: Optional[Sequence[str]], F: int) -> List[str]:
    """one name per variable, default ``var0 ...``"""
    names = [f"var{f}" for f in range(F)] if names is None else list(names)
    if len(names) != F:
        raise ValueError(f"{len(names)} names for {F} variables")
    return names


def datasets(values: torch.Tensor, truth: Optional[torch.Tensor]):
    """The data sets of ``values (..., T, F, H, W)`` -- one per leading index and variable -- and of ``truth (T, F, H, W)`` or None, as
    the kernels read them: ``(x (n_rep, T, F, H W), y (T, F, H W) or None, lead)`` with ``lead`` the leading shape and ``n_rep`` its
    product."""
    if values.dim() < 4:
        raise ValueError(f"values {tuple(values.shape)} must be (..., T, F, H, W)")
    if truth is not None and tuple(truth.shape) != tuple(values.shape[-4:]):
        raise ValueError(f"truth {tuple(truth.shape)} must be {tuple(values.shape[-4:])} = (T, F, H, W) of the values")
    lead = tuple(values.shape[:-4])
    T, F, H, W = (int(s) for s in values.shape[-4:])
    x = dense32(values).view(math.prod(lead), T, F, H * W)
    y = None if truth is None else dense32(truth).view(T, F, H * W)
    return x, y, lead


class VariableReport:
    """What the ``*_report`` functions return: ``names`` and, in their order, one dict of device tensors per variable in ``variables``;
    ``report[name]`` is that variable's dict and iterating gives ``(name, dict)``."""

    def __init__(self, names: Sequence[str], variables: List[dict]):
        self.names, self.variables = list(names), variables

    def __getitem__(self, name: str) -> dict:
        return self.variables[self.names.index(name)]

    def __iter__(self):
        return iter(zip(self.names, self.variables))


def member_mean_std(rows: Sequence[torch.Tensor], keys: Sequence[str]) -> dict:
    """``rows``: one ``(M,)`` device tensor per key -> ``{key: mean, key + "_std": std}`` over the members, as the reference prints them
    (exp/metrics.py:291: numpy's population std); one device-to-host copy"""
    table = torch.stack(list(rows)).cpu().numpy()
    out = {}
    for key, row in zip(keys, table):
        out[key] = float(row.mean())
        out[f"{key}_std"] = float(row.std())
    return out
