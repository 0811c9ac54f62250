"""Multivariate scores of an ensemble on the device: the energy score and the variogram score of the M member FIELDS of every
``(t, f)`` plane against that plane's truth.  ``crps.py`` judges every cell on its own, so an ensemble whose members have the right
marginals and the wrong spatial dependence -- too smooth, too noisy, a front misplaced -- gets a perfect CRPS; spatial dependence is
what a downscaler adds to a coarse observation, and these two scores see it.

``run_ensemble`` leaves ``(M, L, F, H, W)`` on the device, and here it stays there: two HIP kernels (csrc/escore.hip) read every value
once from HBM and serve the pair loop and the stencil from LDS, where torch either forms ``|a|^2 + |b|^2 - 2 a.b`` (on a pressure field
a difference of numbers near ``1e10 H W``, wrong in the first digit in fp32) or keeps an ``(M + 1, M + 1, T, F, H W)`` temporary, and
walks the stencil one sliced pass per offset.

**The definitions**, in this project's words (include/c2w_hip.h: c2w_escore_pairs, c2w_vario_terms); both scores are written from the
papers as recalled (README, statement 10 says what is verified).  fp32 inputs are read as exact numbers.  One ``(t, f)`` plane of
``d = H W`` cells has the rows ``r_0 = y`` (the truth) and ``r_1 .. r_M = x_m``.

*Energy score* (Gneiting & Raftery 2007), the multivariate generalisation of the CRPS:

* ``D2[t, f, p] = sum_c (r_i[c] - r_j[c])^2`` for every pair ``i < j``, ``p`` row-major over ``i < j``, ``P = M (M + 1) / 2`` -- the
  kernel's product, float64 (``pair_sqdist``)
* with ``D = sqrt(D2)``: ``A = (1/M) sum_m D(0, m)^beta``, ``B = sum_{1 <= m < m'} D(m, m')^beta``
* ``ES = A - B / M^2``; the fair form ``A - B / (M (M - 1))``, NaN for ``M = 1``; ``beta`` in ``(0, 2)``, default 1.  For ``d = 1`` and
  ``beta = 1`` this IS the CRPS of ``crps.py``.
* over all variables jointly ``D2_joint[t] = sum_f D2[t, f] / scale_f^2``, ``scale`` given per variable, by default the truth's
  population standard deviation per variable, as ``wasserstein.py`` normalises.  It costs nothing extra.

*Variogram score of order p* (Scheuerer & Hamill 2015), sensitive to the dependence structure where the energy score is weak:

* the offsets ``o = (di, dj)`` with ``max(|di|, |dj|) <= R`` in the half plane ``di > 0``, or ``di == 0 and dj > 0``, row-major;
  ``O = ((2R + 1)^2 - 1) / 2``; ``offsets(radius)`` is the one place that fixes the enumeration
* for every cell pair ``(c, c + o)`` with both cells inside the field ``g_y = |y_c - y_{c+o}|^p`` and
  ``g_x = (1/M) sum_m |x_{m,c} - x_{m,c+o}|^p``
* ``V[t, f, o, 0..2]`` = the sums over the pairs of ``((g_y - g_x)^2, g_y, g_x)`` -- the kernel's product, float64
  (``variogram_terms``)
* ``VS = sum_o w_o V[.., o, 0]`` with ``w`` ``"inverse_distance"`` (``1 / sqrt(di^2 + dj^2)``, the default), ``"uniform"`` or an
  ``(O,)`` tensor, applied here in float64
* ``V[.., 1]`` and ``V[.., 2]`` over the pair count of the offset are the empirical variograms of truth and ensemble
  (``variogram_by_lag``): the figure people plot.

A NaN or an infinity in a row makes every ``D2`` entry of that row NaN in its own ``(t, f)`` entry, and the three sums of every
``(t, f, o)`` one of whose pairs touches its cell; no other entry is touched.

On the GPU the pairs kernel takes ``H W`` a multiple of 4 and ``1 <= M <= 64``; the variogram kernel ``H`` and ``W`` multiples of 8,
``1 <= R <= 8``, ``1 <= M <= 16`` and ``p`` in {0.5, 1, 2}.  Everything else -- other shapes, other ``p``, larger ``M`` or ``R``, CPU
tensors -- takes the same definitions in float64 torch, chunked over time.  Error of the kernels against float64
(tests/fp64_escore_ref.py): ``D2`` within ``3 * 2^-24`` of itself, ``V[.., 0]`` within ``(2M + 8) 2^-24 sum (g_y + g_x)^2``.

Nothing here synchronises.

Out of scope: variogram weights over all cell pairs, more than 16 members on the variogram kernel (the general route takes them),
collectives -- members are rank-local -- and the plotting.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import escore_ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, dense32, scratch, variable_names
from .ensemble_host import on_device as _on_device

NAN = float("nan")
KERNEL_ORDERS = {0.5: 1, 1.0: 2, 2.0: 4}  # p -> the kernel's order2 = 2 p


def offsets(radius: int) -> List[Tuple[int, int]]:
    """The ``O = ((2R + 1)^2 - 1) / 2`` offsets ``(di, dj)`` of radius R in the order every ``O`` axis of this module has: ``(0, 1) ..
    (0, R)``, then ``di = 1 .. R`` each with ``dj = -R .. R``."""
    R = int(radius)
    if R < 1:
        raise ValueError(f"radius {radius} must be at least 1")
    return [(0, dj) for dj in range(1, R + 1)] + [(di, dj) for di in range(1, R + 1) for dj in range(-R, R + 1)]


def pair_index(M: int, i: int, j: int) -> int:
    """where ``pair_sqdist`` puts the pair of rows ``i < j`` (row 0 the truth, row m member m)"""
    return i * (2 * (M + 1) - i - 1) // 2 + (j - i - 1)


# ---------------------------------------------------------------------------------------------------------------- energy score

def _general_pairs(x: torch.Tensor, y: torch.Tensor, d2: torch.Tensor) -> None:
    """The definition for any shape, any M and any device, float64 end to end: x (M, T, F, hw), y (T, F, hw), d2 (T, F, P)."""
    M, T, F, hw = x.shape
    step = chunk_step((M + 1) * F * hw)
    for t0 in range(0, T, step):
        rows = torch.cat([y[None, t0:t0 + step], x[:, t0:t0 + step]]).double()  # (M + 1, t, F, hw)
        bad = ~torch.isfinite(rows).all(dim=-1)                                   # (M + 1, t, F)
        rows = torch.where(bad[..., None], torch.zeros_like(rows), rows)          # the rule below writes those pairs
        p = 0
        for i in range(M):
            d = rows[i + 1:] - rows[i]
            out = (d * d).sum(dim=-1)                                             # (M - i, t, F)
            out = torch.where(bad[i + 1:] | bad[i], torch.full_like(out, NAN), out)
            d2[t0:t0 + step, :, p:p + M - i] = out.permute(1, 2, 0)
            p += M - i


def _launch_pairs(x, y, d2, M, planes, hw) -> bool:
    if not escore_ops.escore_supported(hw, M):
        return False
    return escore_ops.escore_pairs(x, y, d2, scratch(escore_ops.escore_scratch_bytes(planes, hw, M), x.device), M, planes, hw)


def pair_sqdist(samples: torch.Tensor, truth: torch.Tensor) -> torch.Tensor:
    """``samples (M, T, F, H, W)`` against ``truth (T, F, H, W)`` -> ``D2 (T, F, P)`` float64 on the same device: per ``(t, f)`` plane
    the squared Euclidean distance of every pair ``i < j`` of the rows ``truth, member 1 .. member M``, row-major (``pair_index``), so
    the first ``M`` entries are truth against member.  Any float dtype and any strides: a strided or 16-bit input costs one dense fp32
    copy.  No members gives ``P = 0``."""
    check_ensemble(samples, truth, floating=True)
    M, T, F, H, W = (int(s) for s in samples.shape)
    hw = H * W
    x, y = dense32(samples).view(M, T, F, hw), dense32(truth).view(T, F, hw)
    d2 = torch.empty((T, F, M * (M + 1) // 2), dtype=torch.float64, device=x.device)
    if d2.numel() == 0:
        return d2
    if hw == 0:
        return d2.zero_()
    if not (_on_device(x) and _launch_pairs(x, y, d2, M, T * F, hw)):
        _general_pairs(x, y, d2)
    return d2


def _energy_of(d2: torch.Tensor, M: int, beta: float, fair: bool) -> torch.Tensor:
    """(..., P) -> (...): A - B / M^2, or the fair form"""
    if M == 0:
        return torch.full(d2.shape[:-1], NAN, dtype=torch.float64, device=d2.device)
    dist = d2 if beta == 2.0 else torch.sqrt(d2) if beta == 1.0 else d2 ** (beta / 2.0)
    a, b = dist[..., :M].sum(dim=-1) / M, dist[..., M:].sum(dim=-1)
    pairs = M * (M - 1) if fair else M * M
    return a - b / pairs if pairs > 0 else torch.full_like(a, NAN)


def truth_scale(truth: torch.Tensor) -> torch.Tensor:
    """``(F,)`` float64: the truth's population standard deviation per variable over all times and cells -- the default ``scale`` of the
    joint energy score, what ``wasserstein.truth_moments`` divides by."""
    T, F, H, W = (int(s) for s in truth.shape)
    n = T * H * W
    mean = truth.sum(dim=(0, 2, 3), dtype=torch.float64) / n
    ss = torch.zeros(F, dtype=torch.float64, device=truth.device)
    step = chunk_step(F * H * W)
    for i in range(0, T, step):
        ss += ((truth[i:i + step].double() - mean[None, :, None, None]) ** 2).sum(dim=(0, 2, 3))
    return torch.sqrt(ss / n)


def _joint(d2: torch.Tensor, truth: torch.Tensor, scale) -> torch.Tensor:
    """(T, F, P) -> (T, P): the squared distances of the concatenated fields, variable f divided by scale_f"""
    F = int(d2.shape[1])
    if scale is None:
        s = truth_scale(truth)
    else:
        s = torch.as_tensor(scale, dtype=torch.float64, device=d2.device).reshape(-1)
        if s.numel() != F:
            raise ValueError(f"scale has {s.numel()} entries for {F} variables")
    return (d2 / (s * s)[None, :, None]).sum(dim=1)


def _check_beta(beta: float) -> float:
    beta = float(beta)
    if not 0.0 < beta < 2.0:
        raise ValueError(f"beta {beta} must lie in (0, 2)")
    return beta


def energy_score(samples: torch.Tensor, truth: torch.Tensor, *, beta: float = 1.0, fair: bool = False, joint: bool = False,
                 scale=None) -> torch.Tensor:
    """``(T, F)`` float64: the energy score ``A - B / M^2`` of every plane (module docstring), with ``fair=True`` the fair form
    ``A - B / (M (M - 1))`` (NaN for ``M = 1``).  With ``joint=True`` ``(T,)``: the score of all variables as one vector, variable ``f``
    divided by ``scale[f]`` (``(F,)``; default ``truth_scale(truth)``).  No members gives NaN."""
    beta = _check_beta(beta)
    if scale is not None and not joint:
        raise ValueError("scale is the joint score's: pass joint=True")
    d2 = pair_sqdist(samples, truth)
    if joint:
        d2 = _joint(d2, truth, scale)
    return _energy_of(d2, int(samples.shape[0]), beta, fair)


# ---------------------------------------------------------------------------------------------------------------- variogram score

def _check_order(p: float) -> float:
    p = float(p)
    if not (p > 0.0 and math.isfinite(p)):
        raise ValueError(f"order p = {p} must be positive")
    return p


def _power(d: torch.Tensor, p: float) -> torch.Tensor:
    a = d.abs()
    return a if p == 1.0 else torch.sqrt(a) if p == 0.5 else a * a if p == 2.0 else a ** p


def _general_vario(x: torch.Tensor, y: torch.Tensor, V: torch.Tensor, R: int, p: float) -> None:
    """The definition for any shape, any M, R, p and any device, float64 end to end: x (M, T, F, H, W), y (T, F, H, W), V (T, F, O, 3)."""
    M, T, F, H, W = x.shape
    if M == 0:
        V.fill_(NAN)
        return
    step = chunk_step((M + 1) * F * H * W)
    for t0 in range(0, T, step):
        xs, ys = x[:, t0:t0 + step].double(), y[t0:t0 + step].double()
        bad = ~(torch.isfinite(xs).all(dim=0) & torch.isfinite(ys))  # (t, F, H, W)
        xs = torch.where(bad[None], torch.zeros_like(xs), xs)        # the rule below writes those entries
        ys = torch.where(bad, torch.zeros_like(ys), ys)
        for o, (di, dj) in enumerate(offsets(R)):
            if di >= H or abs(dj) >= W:
                V[t0:t0 + step, :, o] = 0.0
                continue
            c = (slice(0, H - di), slice(max(0, -dj), W - max(0, dj)))
            n = (slice(di, H), slice(max(0, dj), W + min(0, dj)))
            gy = _power(ys[..., c[0], c[1]] - ys[..., n[0], n[1]], p)
            gx = _power(xs[..., c[0], c[1]] - xs[..., n[0], n[1]], p).sum(dim=0) / M
            sums = torch.stack([((gy - gx) ** 2).sum(dim=(-2, -1)), gy.sum(dim=(-2, -1)), gx.sum(dim=(-2, -1))], dim=-1)  # (t, F, 3)
            touched = (bad[..., c[0], c[1]] | bad[..., n[0], n[1]]).any(dim=-1).any(dim=-1)
            V[t0:t0 + step, :, o] = torch.where(touched[..., None], torch.full_like(sums, NAN), sums)


def _launch_vario(x, y, V, M, planes, H, W, R, p) -> bool:
    order2 = KERNEL_ORDERS.get(p)
    if order2 is None or not escore_ops.vario_supported(H, W, R, M, order2):
        return False
    return escore_ops.vario_terms(x, y, V, scratch(escore_ops.vario_scratch_bytes(planes, H, W, R), x.device), M, planes, H, W, R, order2)


def variogram_terms(samples: torch.Tensor, truth: torch.Tensor, *, radius: int, p: float = 0.5) -> torch.Tensor:
    """``samples (M, T, F, H, W)`` against ``truth (T, F, H, W)`` -> ``V (T, F, O, 3)`` float64 on the same device: per plane and per
    offset of ``offsets(radius)`` the sums over the cell pairs inside the field of ``((g_y - g_x)^2, g_y, g_x)`` at order ``p`` (module
    docstring).  An offset that does not fit into the field has no pairs and three zeros.  Any float dtype and any strides.  No members
    gives NaN throughout."""
    check_ensemble(samples, truth, floating=True)
    p = _check_order(p)
    offs = offsets(radius)
    M, T, F, H, W = (int(s) for s in samples.shape)
    x, y = dense32(samples), dense32(truth)
    V = torch.empty((T, F, len(offs), 3), dtype=torch.float64, device=x.device)
    if T * F == 0:
        return V
    if H * W == 0:
        return V.zero_() if M else V.fill_(NAN)
    if not (_on_device(x) and _launch_vario(x, y, V, M, T * F, H, W, int(radius), p)):
        _general_vario(x, y, V, int(radius), p)
    return V


def _weights(weights: Union[str, torch.Tensor], radius: int, device) -> torch.Tensor:
    offs = offsets(radius)
    if isinstance(weights, str):
        if weights == "inverse_distance":
            return torch.tensor([1.0 / math.sqrt(di * di + dj * dj) for di, dj in offs], dtype=torch.float64, device=device)
        if weights == "uniform":
            return torch.ones(len(offs), dtype=torch.float64, device=device)
        raise ValueError(f"weights {weights!r} must be 'inverse_distance', 'uniform' or an ({len(offs)},) tensor")
    w = torch.as_tensor(weights, dtype=torch.float64, device=device)
    if tuple(w.shape) != (len(offs),):
        raise ValueError(f"weights {tuple(w.shape)} must be ({len(offs)},) for radius {radius}")
    return w


def _score_of(V: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    # an offset of weight 0 is left out altogether: 0 * NaN would poison the score with an entry the caller has switched off
    return torch.where(w == 0, torch.zeros_like(V[..., 0]), V[..., 0] * w).sum(dim=-1)


def variogram_score(samples: torch.Tensor, truth: torch.Tensor, *, radius: int, p: float = 0.5,
                    weights: Union[str, torch.Tensor] = "inverse_distance") -> torch.Tensor:
    """``(T, F)`` float64: ``sum_o w_o V[t, f, o, 0]``, the variogram score of order ``p`` over the offsets of ``offsets(radius)``;
    ``weights``: ``"inverse_distance"`` (``1 / sqrt(di^2 + dj^2)``), ``"uniform"`` or an ``(O,)`` tensor."""
    w = _weights(weights, radius, samples.device)
    return _score_of(variogram_terms(samples, truth, radius=radius, p=p), w)


def pair_counts(radius: int, H: int, W: int) -> List[int]:
    """per offset of ``offsets(radius)`` the number of cell pairs inside an ``H x W`` field"""
    return [max(0, H - di) * max(0, W - abs(dj)) for di, dj in offsets(radius)]


def _by_lag(V: torch.Tensor, radius: int, H: int, W: int):
    offs = offsets(radius)
    d2 = [di * di + dj * dj for di, dj in offs]
    lags = sorted(set(d2))
    member = torch.tensor([[1.0 if k == lag else 0.0 for lag in lags] for k in d2], dtype=torch.float64, device=V.device)  # (O, L)
    counts = torch.tensor(pair_counts(radius, H, W), dtype=torch.float64, device=V.device) @ member                     # (L,)
    lag = torch.tensor([math.sqrt(k) for k in lags], dtype=torch.float64, device=V.device)
    # an offset without pairs holds zeros; a lag none of whose offsets fits is 0 / 0 = NaN
    return lag, (V[..., 1] @ member) / counts, (V[..., 2] @ member) / counts


def variogram_by_lag(samples: torch.Tensor, truth: torch.Tensor, *, radius: int, p: float = 0.5):
    """``(lag (L,), truth_variogram (T, F, L), ensemble_variogram (T, F, L))`` float64: the empirical variograms of order ``p`` --
    the mean of ``|y_c - y_{c+o}|^p``, and of the member mean of ``|x_c - x_{c+o}|^p``, over all cell pairs at the same distance --
    with the distances ``lag = sqrt(di^2 + dj^2)`` in ascending order."""
    V = variogram_terms(samples, truth, radius=radius, p=p)
    return _by_lag(V, radius, int(truth.shape[2]), int(truth.shape[3]))


# ---------------------------------------------------------------------------------------------------------------- report

class MultivariateReport(VariableReport):
    """Per variable, as device tensors: ``energy``, ``energy_fair``, ``variogram`` (0-d float64, the mean over the times) and
    ``energy_by_time``, ``variogram_by_time (T,)``, ``variogram_truth``, ``variogram_ensemble (L,)`` by ``lag (L,)``.  ``joint`` holds
    the energy score of all variables as one scaled vector: ``energy``, ``energy_fair`` (0-d) and ``energy_by_time (T,)``.  There is no
    joint variogram score: its terms carry the variable's unit to the power ``2 p``."""

    KEYS = ("energy", "energy_fair", "variogram")
    JOINT_KEYS = ("energy", "energy_fair")

    def __init__(self, names: Sequence[str], variables: List[dict], joint: dict, lag: torch.Tensor):
        super().__init__(names, variables)
        self.joint, self.lag = joint, lag

    def as_dict(self, prefix: str = "multivariate") -> dict:
        """flat ``{f"{prefix}/{name}/{key}": float}`` for a logger, ``key`` in ``KEYS``, and ``f"{prefix}/joint/{key}"``, ``key`` in
        ``JOINT_KEYS`` (one device-to-host copy)"""
        if not self.variables:
            return {}
        flat = torch.stack([v[k] for v in self.variables for k in self.KEYS] + [self.joint[k] for k in self.JOINT_KEYS]).cpu().numpy()
        out = {f"{prefix}/{name}/{k}": float(flat[i * len(self.KEYS) + j]) for i, name in enumerate(self.names) for j, k in enumerate(self.KEYS)}
        n = len(self.names) * len(self.KEYS)
        out.update({f"{prefix}/joint/{k}": float(flat[n + j]) for j, k in enumerate(self.JOINT_KEYS)})
        return out


def multivariate_report(samples: torch.Tensor, truth: torch.Tensor, names: Optional[Sequence[str]] = None, *, radius: int = 4, p: float = 0.5,
                        beta: float = 1.0, weights: Union[str, torch.Tensor] = "inverse_distance", scale=None) -> MultivariateReport:
    """The two scores of an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` per variable, from one pass of each
    kernel over the fields.  The fields are expected DE-NORMALISED, as the reference's are: the energy score carries the variable's
    unit, the variogram score its unit to the power ``2 p``; the joint energy score divides variable ``f`` by ``scale[f]`` (default: the
    truth's population standard deviation).  ``names``: one per variable, default ``var0 ...``."""
    check_ensemble(samples, truth, floating=True)
    beta = _check_beta(beta)
    M, T, F, H, W = (int(s) for s in samples.shape)
    names = variable_names(names, F)
    w = _weights(weights, radius, samples.device)
    d2 = pair_sqdist(samples, truth)
    V = variogram_terms(samples, truth, radius=radius, p=p)
    es, fair, vs = _energy_of(d2, M, beta, False), _energy_of(d2, M, beta, True), _score_of(V, w)  # (T, F)
    lag, vario_y, vario_x = _by_lag(V.sum(dim=0), radius, H, W)
    lag_n = max(T, 1)
    variables = [dict(energy=es[:, f].mean(), energy_fair=fair[:, f].mean(), variogram=vs[:, f].mean(), energy_by_time=es[:, f],
                      variogram_by_time=vs[:, f], variogram_truth=vario_y[f] / lag_n, variogram_ensemble=vario_x[f] / lag_n) for f in range(F)]
    dj = _joint(d2, truth, scale)
    ej, ejf = _energy_of(dj, M, beta, False), _energy_of(dj, M, beta, True)
    return MultivariateReport(names, variables, dict(energy=ej.mean(), energy_fair=ejf.mean(), energy_by_time=ej), lag)
