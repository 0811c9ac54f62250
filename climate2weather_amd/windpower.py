"""Wind power of an ensemble on the device: the wind speed at hub height of every member, of the truth and of the coarse observation,
the power a turbine makes of it, their densities and the energy over time -- the reference's downstream application,
``exp/figures.py::_calc_windpower`` (lines 1171-1285) and the ``windpowers`` figure that plots it (:1288 ff.).

The reference takes ``uas`` and ``vas`` of every data set to the host in float64, pushes the speed through ``windpowerlib`` and runs
``2 (M + 2)`` ``scipy`` KDEs.  ``run_ensemble`` leaves ``(M, L, F, H, W)`` on the device, and here it stays there: one HIP kernel
(csrc/wind.hip) reads the two wind planes of every time once, looks the power up in a table held in LDS and sums both per time without
atomics; the densities are ``marginals.gaussian_kde`` on its output.

**The definitions**, in this project's words (include/c2w_hip.h: c2w_wind_power).  One cell has the wind components ``u, v`` in m/s
(fields DE-NORMALISED, as the reference's are):

* ``c = (hub_height / reference_height) ** alpha``, in float64 on the host; the reference's 100, 10, 1/7 are the defaults (:1182-1189)
* ``speed = sqrt(u*u + v*v) * c`` (the reference writes ``np.sqrt(u**2 + v**2)``, not ``hypot``)
* ``power = numpy.interp(speed, xs, ps, left=0, right=0)`` for a curve of ``K >= 2`` knots, ``xs`` strictly increasing, ``ps`` in W:
  ``ps[-1]`` at ``speed == xs[-1]``, 0 strictly above it (cut-out) and below ``xs[0]``, NaN for a NaN speed, 0 for ``+inf``
* per ``(data set, time)`` the sums of both over the ``H W`` cells in float64; mean power ``= S_power / (H W)``; the cumulative energy
  series ``= cumsum_t(mean power / 1e3)``, the reference's :1715 (it plots this divided by its length)

**Recalled, not verified** (README, statement 9): ``windpowerlib`` is not at hand.  That ``ModelChain(turbine).calculate_power_output(wind,
density)`` with its defaults -- ``power_output_model="power_curve"``, ``density_correction=False``, the density argument ignored -- is
the ``numpy.interp`` call above on the turbine's ``power_curve`` table is recalled.  ``numpy.interp`` itself is the float64 reference
of every test.  No turbine's data is shipped: the user passes the curve (a windpowerlib curve as two arrays).

A NaN ``u`` or ``v`` makes its own cell's two values and its own ``(data set, time)`` sums NaN; no other entry is touched.  The kernel
works in fp32: a ``u*u + v*v`` beyond the fp32 range gives speed ``+inf`` (power 0) where the float64 route still has a number.

Nothing here synchronises.

Out of scope: density correction and the ``power_coefficient_curve`` model, logarithmic or Hellmann profiles other than the power law
above, wake and farm models, any turbine's data, the plotting, fusing the KDE into the kernel, and collectives -- members are
rank-local.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import marginals, wind_ops
from .ensemble_host import check_ensemble, chunk_step, dense32, scratch
from .ensemble_host import on_device as _on_device


def hub_factor(hub_height: float = 100.0, reference_height: float = 10.0, alpha: float = 1.0 / 7.0) -> float:
    """``(hub_height / reference_height) ** alpha`` in float64: what a 10 m wind speed is multiplied by to stand for the speed at hub
    height (the power law of the reference, :1186-1189)."""
    hub_height, reference_height, alpha = float(hub_height), float(reference_height), float(alpha)
    if not (hub_height > 0 and reference_height > 0 and np.isfinite([hub_height, reference_height, alpha]).all()):
        raise ValueError(f"hub_height {hub_height}, reference_height {reference_height} must be positive and alpha {alpha} finite")
    return (hub_height / reference_height) ** alpha


class PowerCurve:
    """A turbine's power curve as ``K >= 2`` knots: ``speeds`` in m/s, strictly increasing, ``powers`` in W, both kept in float64.
    ``curve(speed)`` is the definition in float64 on any tensor; the packed table the kernel reads is built once per device."""

    def __init__(self, speeds: Sequence[float], powers: Sequence[float]):
        xs, ps = np.array(speeds, dtype=np.float64), np.array(powers, dtype=np.float64)
        if xs.ndim != 1 or ps.shape != xs.shape or xs.shape[0] < 2:
            raise ValueError(f"speeds {xs.shape} and powers {ps.shape} must be two vectors of the same length K >= 2")
        if not (np.isfinite(xs).all() and np.isfinite(ps).all()):
            raise ValueError("speeds and powers must be finite")
        if not np.all(xs[1:] > xs[:-1]):
            raise ValueError("speeds must increase strictly")
        xs.setflags(write=False), ps.setflags(write=False)
        self.speeds, self.powers = xs, ps
        self._knots, self._tables = {}, {}

    @property
    def K(self) -> int:
        return int(self.speeds.shape[0])

    @property
    def rated(self) -> float:
        """the largest power of the curve, W"""
        return float(self.powers.max())

    @property
    def cut_out(self) -> float:
        """the last knot, m/s: strictly above it the turbine makes nothing"""
        return float(self.speeds[-1])

    def _on(self, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        key = str(device)
        if key not in self._knots:
            xs, ps = torch.from_numpy(self.speeds.copy()).to(device), torch.from_numpy(self.powers.copy()).to(device)
            self._knots[key] = (xs, ps, (ps[1:] - ps[:-1]) / (xs[1:] - xs[:-1]))
        return self._knots[key]

    def device_table(self, device) -> Optional[torch.Tensor]:
        """the kernel's packed table (include/c2w_hip.h: c2w_wind_table) as a uint8 tensor on ``device``, cached; None where the
        library refuses the curve (more than 256 knots, or knots that collapse in fp32): such a curve takes the general route"""
        key = str(device)
        if key not in self._tables:
            host = wind_ops.wind_table(self.speeds, self.powers)
            self._tables[key] = None if host is None else torch.from_numpy(host.copy()).to(device)
        return self._tables[key]

    def __call__(self, speed: torch.Tensor) -> torch.Tensor:
        """``numpy.interp(speed, speeds, powers, left=0, right=0)`` in float64, on the device of ``speed``"""
        s = speed.to(torch.float64)
        xs, ps, slope = self._on(s.device)
        j = (torch.bucketize(s, xs, right=True) - 1).clamp_(0, self.K - 2)  # the knots at or below s, less one
        val = ps[j] + (s - xs[j]) * slope[j]
        val = torch.where(s == xs[-1], ps[-1], val)
        return torch.where((s < xs[0]) | (s > xs[-1]), torch.zeros_like(val), val)  # a NaN speed compares false: it stays NaN


def _general(x: torch.Tensor, curve: PowerCurve, u: int, v: int, c: float, derived: Optional[torch.Tensor], sums: torch.Tensor) -> None:
    """The definition for any shape, any curve and any device, float64 end to end: x (P, F, hw), derived (P, 2, hw) or None, sums
    (P, 2)."""
    P, F, hw = x.shape
    step = chunk_step(hw)
    for i in range(0, P, step):
        uu, vv = x[i:i + step, u].double(), x[i:i + step, v].double()
        speed = torch.sqrt(uu * uu + vv * vv) * c
        power = curve(speed)
        sums[i:i + step, 0], sums[i:i + step, 1] = speed.sum(dim=-1), power.sum(dim=-1)
        if derived is not None:
            derived[i:i + step, 0], derived[i:i + step, 1] = speed.to(derived.dtype), power.to(derived.dtype)


def _launch(x, F, u, v, curve, c, sums, derived, planes, hw) -> bool:
    if not wind_ops.wind_supported(hw, curve.K):
        return False
    table = curve.device_table(x.device)
    if table is None:
        return False
    ws = scratch(wind_ops.wind_scratch_bytes(planes, hw), x.device)
    return wind_ops.wind_power(x, F, u, v, table, curve.K, c, sums, derived, ws, planes, hw)


def _check(values: torch.Tensor, curve: PowerCurve, u: int, v: int) -> None:
    if values.dim() < 4:
        raise ValueError(f"values {tuple(values.shape)} must be (..., T, F, H, W)")
    if not values.is_floating_point():
        raise ValueError(f"values ({values.dtype}) must be floating point")
    if not isinstance(curve, PowerCurve):
        raise ValueError("curve must be a PowerCurve")
    F = int(values.shape[-3])
    for name, i in (("u", u), ("v", v)):
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < F:
            raise ValueError(f"{name} = {i!r} must be the index of a variable, 0 .. {F - 1}")


def wind_fields(values: torch.Tensor, curve: PowerCurve, *, u: int, v: int, hub_height: float = 100.0, reference_height: float = 10.0,
                alpha: float = 1.0 / 7.0, maps: bool = True):
    """``values (..., T, F, H, W)`` with the wind components in variables ``u`` and ``v`` -> ``(derived (..., T, 2, H, W) fp32, sums
    (..., T, 2) float64)`` on the same device: per cell the hub-height speed (plane 0) and the power (plane 1), per time their sums over
    the cells (module docstring).  ``maps=False`` gives ``(None, sums)`` and writes no per-cell values.  ``derived`` is the layout
    ``marginals.gaussian_kde`` takes as two variables.  Any float dtype and any strides: a strided or 16-bit input costs one dense fp32
    copy.

    On the GPU, ``H W`` a multiple of 4 and a curve of at most 256 knots take the kernel; everything else and CPU tensors take the same
    definition in float64."""
    _check(values, curve, u, v)
    c = hub_factor(hub_height, reference_height, alpha)
    lead = tuple(int(s) for s in values.shape[:-3])  # (..., T)
    F, H, W = (int(s) for s in values.shape[-3:])
    hw = H * W
    planes = int(np.prod(lead, dtype=np.int64)) if lead else 1
    x = dense32(values).view(planes, F, hw)
    sums = torch.empty((planes, 2), dtype=torch.float64, device=x.device)
    derived = torch.empty((planes, 2, hw), dtype=torch.float32, device=x.device) if maps else None
    if planes * hw == 0:
        sums.zero_()
    elif not (_on_device(x) and _launch(x, F, u, v, curve, c, sums, derived, planes, hw)):
        _general(x, curve, u, v, c, derived, sums)
    return (derived.view(lead + (2, H, W)) if maps else None), sums.view(lead + (2,))


def mean_power(values: torch.Tensor, curve: PowerCurve, *, u: int, v: int, **hub) -> torch.Tensor:
    """``(..., T)`` float64: the mean power over the cells of every time, W"""
    _, sums = wind_fields(values, curve, u=u, v=v, maps=False, **hub)
    return sums[..., 1] / (int(values.shape[-2]) * int(values.shape[-1]))


def _energy_of(mean: torch.Tensor) -> torch.Tensor:
    return torch.cumsum(mean / 1e3, dim=-1)


def cumulative_energy(values: torch.Tensor, curve: PowerCurve, *, u: int, v: int, **hub) -> torch.Tensor:
    """``(..., T)`` float64: ``cumsum_t(mean power / 1e3)``, the series of the reference's figure (:1715, which plots it divided by its
    length)"""
    return _energy_of(mean_power(values, curve, u=u, v=v, **hub))


class WindReport:
    """The entries of the reference's ``windpower.npz`` (:1259-1278) as device tensors, by their names there -- for each of ``sample``,
    ``gt`` and (with an observation) ``obs``: ``_windspeed_100`` and ``_windpower`` (fp32, per cell), ``_windspeed_kde`` and
    ``_windpower_kde`` (float64, at the grids), ``_power_gen`` (the curve at the speed grid times the speed density); and
    ``windspeed_range``, ``windpower_range``, ``power_curve``.  Additionally ``_mean_power`` and ``_cumulative_energy`` per time."""

    def __init__(self, data: dict, rated: float):
        self.data, self.rated = data, rated

    def __getitem__(self, key: str) -> torch.Tensor:
        return self.data[key]

    def __contains__(self, key: str) -> bool:
        return key in self.data

    def __iter__(self):
        return iter(self.data)

    def keys(self):
        return self.data.keys()

    def as_dict(self, prefix: str = "wind") -> dict:
        """flat ``{f"{prefix}/{set}/{key}": float}`` for a logger, ``set`` in sample / gt / obs, ``key`` in mean_power (W, over all
        times, for the samples over all members too) and capacity_factor (that over the curve's rated power); one device-to-host copy"""
        sets = [s for s in ("sample", "gt", "obs") if f"{s}_mean_power" in self.data]
        means = torch.stack([self.data[f"{s}_mean_power"].mean() for s in sets]).cpu().numpy()
        out = {}
        for s, m in zip(sets, means):
            out[f"{prefix}/{s}/mean_power"] = float(m)
            out[f"{prefix}/{s}/capacity_factor"] = float(m) / self.rated if self.rated != 0 else float("nan")
        return out


def _kdes(derived: torch.Tensor, grids: Sequence[torch.Tensor], bw_method, truth: Optional[torch.Tensor] = None):
    """densities of speed and of power: [(values' (..., N_s), truth's (N_s,) or None), (..., N_p) ...]; one call where both grids have
    the same length"""
    if int(grids[0].shape[0]) == int(grids[1].shape[0]):
        got = marginals.gaussian_kde(derived, torch.stack(list(grids)), bw_method=bw_method, truth=truth)
        a, b = got if truth is not None else (got, None)
        return [(a[..., f, :], None if b is None else b[f]) for f in range(2)]
    out = []
    for f in range(2):
        got = marginals.gaussian_kde(derived[..., f:f + 1, :, :], grids[f][None], bw_method=bw_method,
                                     truth=None if truth is None else truth[:, f:f + 1])
        a, b = got if truth is not None else (got, None)
        out.append((a[..., 0, :], None if b is None else b[0]))
    return out


def wind_report(samples: torch.Tensor, truth: torch.Tensor, curve: PowerCurve, *, u: int = 2, v: int = 3,
                observation: Optional[torch.Tensor] = None, speed_grid: Optional[torch.Tensor] = None,
                power_grid: Optional[torch.Tensor] = None, location: Optional[Tuple[int, int]] = None, bw_method="scott",
                hub_height: float = 100.0, reference_height: float = 10.0, alpha: float = 1.0 / 7.0) -> WindReport:
    """What ``_calc_windpower`` computes, for an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` and, if given, the
    coarse ``observation (L', F, h, w)``, all DE-NORMALISED with the wind components in variables ``u`` and ``v`` (``uas``, ``vas``).
    The grids default to the reference's ``linspace(0, 30, 300)`` m/s and to ``linspace(0, curve.rated, 300)`` W (the reference
    hard-codes 3e6, the rated power of its turbine).  ``location=(rlat, rlon)`` looks at one cell, as the reference's
    ``single_location`` does: the cell is sliced first, the observation at both indices divided by ``H // h`` (:1204-1208), and the
    per-cell entries lose their two cell dimensions.  The densities come from ``marginals.gaussian_kde``: members and truth in one call,
    the observation in its own."""
    check_ensemble(samples, truth, time="L")
    F = int(truth.shape[1])
    if observation is not None and (observation.dim() != 4 or int(observation.shape[1]) != F):
        raise ValueError(f"observation {tuple(observation.shape)} must be (L', F = {F}, h, w)")
    _check(samples, curve, u, v), _check(truth, curve, u, v)
    dev = samples.device
    if location is not None:
        rlat, rlon = (int(i) for i in location)
        H, W = int(truth.shape[-2]), int(truth.shape[-1])
        if not (0 <= rlat < H and 0 <= rlon < W):
            raise ValueError(f"location {location} outside the {H} x {W} cells")
        samples, truth = samples[..., rlat:rlat + 1, rlon:rlon + 1], truth[..., rlat:rlat + 1, rlon:rlon + 1]
        if observation is not None:
            k = max(1, H // int(observation.shape[-2]))
            observation = observation[..., rlat // k:rlat // k + 1, rlon // k:rlon // k + 1]
    ws = torch.linspace(0.0, 30.0, 300, dtype=torch.float64, device=dev) if speed_grid is None else speed_grid.to(device=dev, dtype=torch.float64)
    wp = torch.linspace(0.0, curve.rated, 300, dtype=torch.float64, device=dev) if power_grid is None else power_grid.to(device=dev, dtype=torch.float64)
    if ws.dim() != 1 or wp.dim() != 1 or ws.numel() < 1 or wp.numel() < 1:
        raise ValueError("speed_grid and power_grid must be vectors")
    hub = dict(hub_height=hub_height, reference_height=reference_height, alpha=alpha)
    power_curve = curve(ws)
    data = dict(windspeed_range=ws, windpower_range=wp, power_curve=power_curve)

    def put(name, derived, sums, kdes):
        speed, power = derived[..., 0, :, :], derived[..., 1, :, :]
        if location is not None:
            speed, power = speed[..., 0, 0], power[..., 0, 0]
        data[f"{name}_windspeed_100"], data[f"{name}_windpower"] = speed, power
        data[f"{name}_windspeed_kde"], data[f"{name}_windpower_kde"] = kdes
        data[f"{name}_power_gen"] = power_curve * kdes[0]
        mean = sums[..., 1] / (int(derived.shape[-2]) * int(derived.shape[-1]))
        data[f"{name}_mean_power"], data[f"{name}_cumulative_energy"] = mean, _energy_of(mean)

    d_s, s_s = wind_fields(samples, curve, u=u, v=v, **hub)
    d_t, s_t = wind_fields(truth, curve, u=u, v=v, **hub)
    (ks_s, ks_t), (kp_s, kp_t) = _kdes(d_s, (ws, wp), bw_method, truth=d_t)
    put("sample", d_s, s_s, (ks_s, kp_s))
    put("gt", d_t, s_t, (ks_t, kp_t))
    if observation is not None:
        d_o, s_o = wind_fields(observation, curve, u=u, v=v, **hub)
        (ks_o, _), (kp_o, _) = _kdes(d_o, (ws, wp), bw_method)
        put("obs", d_o, s_o, (ks_o, kp_o))
    return WindReport(data, curve.rated)
