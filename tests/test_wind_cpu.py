"""CPU checks of the ensemble wind power (climate2weather_amd.windpower): both routes of every public function -- the general float64
one and the launcher's, with tests/emu_wind_ops.py standing in for the HIP kernels -- against numpy.interp in float64 by the rule of
tests/fp64_wind_ref.py, the curve's validation and end rules, the derived series and the report against a plain numpy / scipy
restatement of the reference's lines, the argument checks, the library's table builder against its Python restatement, the kernels' own
table, lookup, index maps and arithmetic compiled for the host (csrc/wind_core.h) under the address and undefined-behaviour
sanitizers, and the C declarations against the ctypes prototypes."""
import os
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_wind_ops
import fp64_wind_ref as R
import host_program
from climate2weather_amd import _lib
from climate2weather_amd import wind_ops
from climate2weather_amd import windpower as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME_HEIGHT = dict(hub_height=10.0, reference_height=10.0)  # hub factor 1: the on_knots kind


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of windpower.wind_fields on CPU tensors"""
    if request.param == "launcher":
        emu_wind_ops.install(monkeypatch, wind_ops, W)
    return request.param


def _curve(name):
    return W.PowerCurve(*R.curve(name))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))


def _heights(kind):
    return SAME_HEIGHT if kind == "on_knots" else {}


def knots_expected(ref, u, v):
    """on_knots: (mask of the cells whose speed is a table knot or lies one fp32 beyond an end, the power expected there exactly):
    fp32(ps[j]) at x^_j, 0 one fp32 below x^_0 and one above x^_{K-1}"""
    a = np.abs(ref.x[:, :, u])
    x32, p32 = ref.xs.astype(np.float32), ref.ps.astype(np.float32)
    j = np.clip(np.searchsorted(x32, a), 0, x32.shape[0] - 1)
    at_knot = x32[j] == a
    outside = (a == np.nextafter(x32[0], np.float32(-np.inf))) | (a == np.nextafter(x32[-1], np.float32(np.inf)))
    return at_knot | outside, np.where(at_knot, p32[j], np.float32(0))


# ------------------------------------------------------------------------------------------------------------------ the definition

SHAPES = [(1, 1, 4, 2, 2, 2, 3), (3, 2, 2, 8, 8, 1, 0), (2, 3, 4, 16, 12, 2, 3), (2, 2, 4, 41, 100, 2, 3)]


@pytest.mark.parametrize("D,T,F,H,W_,u,v", SHAPES)
def test_every_kind_and_curve_against_numpy_interp(route, D, T, F, H, W_, u, v):
    """hw = 4, 64, 192 and 4100 (two chunks of the launcher's, the second of four cells); F = 2 with (u, v) = (1, 0) fails a swapped or
    wrong plane index (the other variables lie near 1000)"""
    worst = {}
    for name in R.CURVES:
        curve = _curve(name)
        for kind in R.KINDS:
            ref = R.reference(kind, name, D, T, F, H * W_, u, v)
            derived, sums = W.wind_fields(torch.tensor(ref.x).view(D, T, F, H, W_), curve, u=u, v=v, **_heights(kind))
            assert derived.dtype == torch.float32 and derived.shape == (D, T, 2, H, W_) and sums.dtype == torch.float64 and sums.shape == (D, T, 2)
            got = derived.numpy().reshape(D, T, 2, -1)
            if route == "general" and kind == "huge":  # float64 has no overflow: a number where the kernel says inf, power 0 either way
                want = np.sqrt(ref.x[:, :, u].astype(np.float64) ** 2 + ref.x[:, :, v].astype(np.float64) ** 2) * ref.c
                assert np.allclose(got[:, :, 0], want, rtol=2 * R.EPS, atol=0) and np.all(got[:, :, 1] == 0) and np.all(sums.numpy()[..., 1] == 0)
                continue
            (rs, ok_s), (rp, ok_p) = R.worst_speed(got[:, :, 0], ref), R.worst_power(got[:, :, 1], ref)
            (rss, ok_ss), (rsp, ok_sp) = R.worst_sums(sums.numpy(), ref)
            worst[kind] = np.maximum(worst.get(kind, np.zeros(4)), [rs, rp, rss, rsp])
            assert ok_s and ok_p and ok_ss and ok_sp, (name, kind, rs, rp, rss, rsp)
            assert _same_bits(W.wind_fields(torch.tensor(ref.x).view(D, T, F, H, W_), curve, u=u, v=v, maps=False, **_heights(kind))[1].numpy(),
                              sums.numpy())  # without the maps: the same sums
            if kind == "on_knots" and route == "launcher":
                mask, want = knots_expected(ref, u, v)
                assert mask.mean() > 0.3 and np.array_equal(got[:, :, 1][mask], want[mask])
                assert np.array_equal(got[:, :, 0], np.abs(ref.x[:, :, u]))  # the speeds are exact
    print(f"{route} {(D, T, F, H * W_)}: error over bound (limit 1), speed / power / speed sums / power sums: " +
          "; ".join(f"{k} " + " / ".join(f"{x:.3g}" for x in w) for k, w in worst.items()))


def test_the_rule_refuses_a_wrong_interval_and_a_wrong_plane():
    """the negative control: the neighbouring interval's line, and u taken from the wrong variable, fail the rule"""
    ref = R.reference("typical", "k61", 2, 2, 4, 64, 2, 3)
    xs, ps = ref.xs, ref.ps
    j = np.clip(np.searchsorted(xs, ref.speed, side="right") - 1, 0, xs.shape[0] - 2)
    wrong = np.clip(j + 1, 0, xs.shape[0] - 2)
    slope = (ps[1:] - ps[:-1]) / (xs[1:] - xs[:-1])
    live = (ref.speed >= xs[0]) & (ref.speed < xs[-1])
    off = np.where(live, ps[wrong] + (ref.speed - xs[wrong]) * slope[wrong], 0.0)
    assert not R.worst_power(off, ref)[1] and R.worst_power(ref.power, ref)[1]
    swapped = R.speed64(ref.x[:, :, 1], ref.x[:, :, 3], ref.c)
    assert not R.worst_speed(swapped, ref)[1] and R.worst_speed(ref.speed.astype(np.float32), ref)[1]


# ------------------------------------------------------------------------------------------------------------------ the curve

def test_power_curve_validation_and_properties():
    c = W.PowerCurve([3.0, 12.0, 25.0], [0.0, 2.0e6, 1.5e6])
    assert c.K == 3 and c.rated == 2.0e6 and c.cut_out == 25.0 and c.speeds.dtype == np.float64 and c.powers.dtype == np.float64
    for xs, ps in (([3.0], [1.0]), ([3.0, 3.0], [0.0, 1.0]), ([3.0, 2.0], [0.0, 1.0]), ([1.0, 2.0, 3.0], [0.0, 1.0]), ([1.0, np.nan], [0.0, 1.0]),
                   ([1.0, 2.0], [0.0, np.inf]), ([[1.0, 2.0]], [[0.0, 1.0]])):
        with pytest.raises(ValueError):
            W.PowerCurve(xs, ps)
    with pytest.raises(ValueError):
        c.speeds[0] = 1.0  # the knots are the curve's: read-only
    assert W.hub_factor() == (100.0 / 10.0) ** (1.0 / 7.0) and W.hub_factor(10.0, 10.0) == 1.0 and W.hub_factor(80.0, 10.0, 0.2) == 8.0 ** 0.2
    for bad in ((0.0, 10.0, 0.1), (100.0, -1.0, 0.1), (100.0, 10.0, float("nan"))):
        with pytest.raises(ValueError):
            W.hub_factor(*bad)


def test_the_curve_in_float64_is_numpy_interp():
    rng = np.random.default_rng(5)
    for name in R.CURVES:
        xs, ps = R.curve(name)
        s = np.concatenate([rng.uniform(-1.0, 40.0, 4000), xs, np.nextafter(xs, np.inf), np.nextafter(xs, -np.inf), [np.inf, -np.inf, np.nan, 0.0]])
        got = _curve(name)(torch.tensor(s)).numpy()
        want = np.interp(s, xs, ps, left=0.0, right=0.0)
        assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.allclose(got, want, rtol=1e-13, atol=1e-9 * R.RATED, equal_nan=True)  # the slope is formed first, as numpy forms it
        at = np.isin(s, xs)
        assert np.array_equal(got[at], want[at]) and np.array_equal(got[~np.isnan(s) & ((s < xs[0]) | (s > xs[-1]))], np.zeros(np.sum((s < xs[0]) | (s > xs[-1]))))


def test_the_end_rules(route):
    """== xs[-1] gives ps[-1]; strictly above gives 0; below xs[0] gives 0; NaN gives NaN; +inf gives 0 -- with hub factor 1 and v = 0 the
    speeds are exact"""
    xs, ps = np.array([3.0, 12.0, 25.0]), np.array([1.0e5, 2.0e6, 1.5e6])
    curve = W.PowerCurve(xs, ps)
    f32 = np.float32
    u = np.array([25.0, np.nextafter(f32(25.0), f32(np.inf)), np.nextafter(f32(3.0), f32(-np.inf)), np.nan, np.inf, 3.0, -25.0, 0.0], f32)
    x = np.zeros((1, 2, 8), f32)
    x[0, 1] = u
    derived, sums = W.wind_fields(torch.tensor(x).view(1, 2, 2, 4), curve, u=1, v=0, **SAME_HEIGHT)
    got = derived.numpy().reshape(2, 8)
    assert _same_bits(got[0], np.abs(u)) and _same_bits(got[1], np.array([1.5e6, 0.0, 0.0, np.nan, 0.0, 1.0e5, 1.5e6, 0.0], f32))
    assert torch.isnan(sums).all()
    x[0, 1, 3] = 1.0
    _, sums = W.wind_fields(torch.tensor(x).view(1, 2, 2, 4), curve, u=1, v=0, **SAME_HEIGHT)
    assert float(sums[0, 0]) == np.inf and float(sums[0, 1]) == 1.5e6 + 1.0e5 + 1.5e6


# ------------------------------------------------------------------------------------------------------------------ series and report

def test_derived_series_are_the_reference_s_numpy_lines(route):
    D, T, F, H, W_ = 3, 5, 4, 8, 8
    ref = R.reference("typical", "k61", D, T, F, H * W_, 2, 3)
    curve, X = _curve("k61"), torch.tensor(ref.x).view(D, T, F, H, W_)
    derived, sums = W.wind_fields(X, curve, u=2, v=3)
    power = derived[:, :, 1].numpy().astype(np.float64)
    mean, energy = W.mean_power(X, curve, u=2, v=3), W.cumulative_energy(X, curve, u=2, v=3)
    assert mean.shape == (D, T) and energy.shape == (D, T) and mean.dtype == torch.float64 and energy.dtype == torch.float64
    rtol = 1e-12 if route == "launcher" else 2 * R.EPS  # the general route sums in float64 what it then rounds to fp32 per cell
    for d in range(D):
        gwp = np.cumsum(power[d].mean((-2, -1)) / 1e3)  # the reference's line, on this route's own per-cell powers
        assert np.allclose(energy[d].numpy(), gwp, rtol=rtol, atol=0) and np.allclose(mean[d].numpy(), power[d].mean((-2, -1)), rtol=rtol, atol=0)
    want_mean, want_energy = R.series64(ref.sums, H * W_)
    lo, hi = R.series64(np.stack([ref.sums[..., 0], ref.s_lo], -1), H * W_), R.series64(np.stack([ref.sums[..., 0], ref.s_hi], -1), H * W_)
    assert np.all((lo[0] <= mean.numpy()) & (mean.numpy() <= hi[0]))  # and against float64 by the rule for the sums
    assert np.all((lo[1] * (1 - 1e-12) <= energy.numpy()) & (energy.numpy() <= hi[1] * (1 + 1e-12)))
    assert np.allclose(mean.numpy(), want_mean, rtol=1e-5) and np.allclose(energy.numpy(), want_energy, rtol=1e-5)
    assert torch.equal(W.mean_power(X[0], curve, u=2, v=3), mean[0])  # any leading dimensions


def calc_windpower(samples, gt, obs, xs, ps, u, v, ws_range, wp_range, location=None):
    """the reference's _calc_windpower (exp/figures.py:1171-1285) restated in plain numpy / scipy on (M, L, F, H, W), (L, F, H, W),
    (L', F, h, w) arrays, with numpy.interp in the place of windpowerlib (README, statement 9)"""
    from scipy.stats import gaussian_kde
    if location is not None:
        rlat, rlon = location
        k = gt.shape[-2] // obs.shape[-2]
        samples, gt, obs = samples[..., rlat, rlon], gt[..., rlat, rlon], obs[..., rlat // k, rlon // k]
    fac = (100 / 10) ** (1 / 7)

    def hub(x):
        return (np.sqrt(x[..., u, :, :] ** 2 + x[..., v, :, :] ** 2) * fac if location is None else np.sqrt(x[..., u] ** 2 + x[..., v] ** 2) * fac).astype(np.float32)

    def power(s):
        return np.interp(s, xs, ps, left=0.0, right=0.0)

    out = {}
    curve = power(ws_range)
    for name, x in (("sample", samples.astype(np.float64)), ("gt", gt.astype(np.float64)), ("obs", obs.astype(np.float64))):
        speed = hub(x)
        pw = power(speed).astype(np.float32)
        sets = [(speed[i], pw[i]) for i in range(speed.shape[0])] if name == "sample" else [(speed, pw)]
        ks = np.stack([gaussian_kde(s.reshape(-1))(ws_range) for s, _ in sets])
        kp = np.stack([gaussian_kde(p.reshape(-1))(wp_range) for _, p in sets])
        if name != "sample":
            ks, kp = ks[0], kp[0]
        out.update({f"{name}_windspeed_100": speed, f"{name}_windpower": pw, f"{name}_windspeed_kde": ks, f"{name}_windpower_kde": kp,
                    f"{name}_power_gen": curve * ks})
    out.update(windpower_range=wp_range, windspeed_range=ws_range, power_curve=curve)
    return out


REPORT_KEYS = {f"{s}_{k}" for s in ("sample", "gt", "obs") for k in ("windspeed_100", "windpower", "windspeed_kde", "windpower_kde", "power_gen",
                                                                     "mean_power", "cumulative_energy")} | {"windspeed_range", "windpower_range", "power_curve"}


def _report_inputs(M=3, L=4, F=4, H=8, W_=8, h=2):
    rng = np.random.default_rng(11)
    base = 6.0 * rng.standard_normal((L, F, H, W_))
    gt = (base + 2.0 * rng.standard_normal((L, F, H, W_))).astype(np.float32)
    samples = (base[None] + 2.0 * rng.standard_normal((M, L, F, H, W_))).astype(np.float32)
    obs = gt.reshape(L, F, h, H // h, h, W_ // h).mean(axis=(3, 5)).astype(np.float32)
    return samples, gt, obs


def test_report_keys_shapes_and_values_against_the_restated_reference(route):
    M, L, F, H, W_, h = 3, 4, 4, 8, 8, 2
    samples, gt, obs = _report_inputs(M, L, F, H, W_, h)
    xs, ps = R.curve("k61")
    curve = W.PowerCurve(xs, ps)
    rep = W.wind_report(torch.tensor(samples), torch.tensor(gt), curve, observation=torch.tensor(obs))
    want = calc_windpower(samples, gt, obs, xs, ps, 2, 3, np.linspace(0.0, 30.0, 300), np.linspace(0.0, curve.rated, 300))
    assert set(rep.keys()) == REPORT_KEYS and set(want) <= set(rep.keys())
    for key, val in want.items():
        got = rep[key].numpy()
        assert got.shape == val.shape, key
        if key.endswith("_windspeed_100"):
            assert got.dtype == np.float32 and np.allclose(got, val, rtol=8 * R.EPS, atol=0), key
        elif key.endswith("_windpower"):
            assert got.dtype == np.float32 and np.allclose(got, val, rtol=1e-4, atol=1e-6 * R.RATED), key  # the exact rule: the test above
        else:
            # a density of n values smooths a per-value error e into e / h of itself: 1e-6 relative on the values, 1e-4 allowed here
            assert got.dtype == np.float64 and np.allclose(got, val, rtol=1e-4, atol=1e-4 * np.abs(val).max()), key
    rtol = 1e-12 if route == "launcher" else 2 * R.EPS  # the general route sums in float64 what it then rounds to fp32 per cell
    for name in ("sample", "gt", "obs"):  # the observation is 2 x 2: the general route on either side
        power = rep[f"{name}_windpower"].numpy().astype(np.float64)
        assert np.allclose(rep[f"{name}_mean_power"].numpy(), power.mean((-2, -1)), rtol=2 * R.EPS if name == "obs" else rtol)
        assert np.allclose(rep[f"{name}_cumulative_energy"].numpy(), np.cumsum(power.mean((-2, -1)) / 1e3, axis=-1), rtol=2 * R.EPS if name == "obs" else rtol)
    assert rep["sample_mean_power"].shape == (M, L) and rep["gt_cumulative_energy"].shape == (L,) and rep["obs_mean_power"].shape == (L,)
    flat = rep.as_dict()
    assert set(flat) == {f"wind/{s}/{k}" for s in ("sample", "gt", "obs") for k in ("mean_power", "capacity_factor")}
    assert flat["wind/gt/mean_power"] == pytest.approx(float(rep["gt_mean_power"].mean()), rel=1e-14)
    assert flat["wind/sample/capacity_factor"] == pytest.approx(float(rep["sample_mean_power"].mean()) / curve.rated, rel=1e-14)
    assert all(isinstance(x, float) for x in flat.values()) and "eval/obs/capacity_factor" in rep.as_dict("eval")
    no_obs = W.wind_report(torch.tensor(samples), torch.tensor(gt), curve)
    assert set(no_obs.keys()) == {k for k in REPORT_KEYS if not k.startswith("obs_")} and set(no_obs.as_dict()) == {k for k in flat if "/obs/" not in k}
    grids = W.wind_report(torch.tensor(samples), torch.tensor(gt), curve, speed_grid=torch.linspace(0, 20, 7), power_grid=torch.linspace(0, 1e6, 5))
    assert grids["sample_windspeed_kde"].shape == (M, 7) and grids["gt_windpower_kde"].shape == (5,) and grids["power_curve"].shape == (7,)
    assert np.allclose(grids["gt_windspeed_kde"].numpy(), calc_windpower(samples, gt, obs, xs, ps, 2, 3, np.linspace(0, 20, 7), np.linspace(0, 1e6, 5))["gt_windspeed_kde"], rtol=1e-4)


def test_report_at_one_location():
    """location=(rlat, rlon): one cell of the fields, the observation at both indices divided by H // h; the general route"""
    M, L, F, H, W_, h = 3, 12, 4, 8, 8, 2
    samples, gt, obs = _report_inputs(M, L, F, H, W_, h)
    xs, ps = R.curve("k3")
    curve = W.PowerCurve(xs, ps)
    rep = W.wind_report(torch.tensor(samples), torch.tensor(gt), curve, observation=torch.tensor(obs), location=(5, 2))
    want = calc_windpower(samples, gt, obs, xs, ps, 2, 3, np.linspace(0.0, 30.0, 300), np.linspace(0.0, curve.rated, 300), location=(5, 2))
    assert rep["sample_windspeed_100"].shape == (M, L) and rep["gt_windpower"].shape == (L,) and rep["obs_windspeed_100"].shape == (L,)
    fac = (100 / 10) ** (1 / 7)
    assert np.allclose(rep["obs_windspeed_100"].numpy(), np.sqrt(obs[:, 2, 1, 0].astype(np.float64) ** 2 + obs[:, 3, 1, 0].astype(np.float64) ** 2) * fac, rtol=1e-6)
    for key, val in want.items():
        assert np.allclose(rep[key].numpy(), val, rtol=1e-4, atol=1e-4 * max(1e-30, np.abs(val).max())), key
    assert rep["gt_mean_power"].shape == (L,) and np.allclose(rep["gt_mean_power"].numpy(), rep["gt_windpower"].numpy().astype(np.float64))
    with pytest.raises(ValueError):
        W.wind_report(torch.tensor(samples), torch.tensor(gt), curve, location=(8, 0))


# ------------------------------------------------------------------------------------------------------------------ the interface

def test_any_dtype_any_strides(route):
    base = 8.0 * torch.randn(2, 3, 4, 8, 16, dtype=torch.float64)
    view = base[..., ::2]  # strided
    curve = _curve("k61")
    for cast in (torch.float64, torch.float16, torch.bfloat16):
        X = view.to(cast)
        dense = X.float().contiguous()
        derived, sums = W.wind_fields(X, curve, u=2, v=3)
        d2, s2 = W.wind_fields(dense, curve, u=2, v=3)
        assert torch.equal(derived, d2) and torch.equal(sums, s2) and derived.shape == (2, 3, 2, 8, 8), cast
        x32 = dense.numpy()
        s64 = R.speed64(x32[:, :, 2].reshape(2, 3, 64), x32[:, :, 3].reshape(2, 3, 64), R.hub_factor())
        assert np.allclose(derived[:, :, 0].numpy().reshape(2, 3, 64), s64, rtol=8 * R.EPS, atol=0)
        assert np.allclose(sums[..., 1].numpy(), R.power64(s64, *R.curve("k61")).sum(-1), rtol=1e-5)


def test_argument_checks():
    x, curve = torch.zeros(2, 3, 4, 8, 8), _curve("k2")
    for fn in (W.wind_fields, W.mean_power, W.cumulative_energy):
        with pytest.raises(ValueError):
            fn(x[0, 0, 0], curve, u=0, v=1)          # no (T, F, H, W)
        with pytest.raises(ValueError):
            fn(x.long(), curve, u=0, v=1)
        with pytest.raises(ValueError, match="0 .. 3"):
            fn(x, curve, u=4, v=1)
        with pytest.raises(ValueError):
            fn(x, curve, u=0, v=-1)
        with pytest.raises(ValueError):
            fn(x, (R.curve("k2")), u=0, v=1)       # two arrays are not a PowerCurve
        with pytest.raises(ValueError):
            fn(x, curve, u=0, v=1, hub_height=0.0)
        with pytest.raises(TypeError):
            fn(x, curve)                             # u and v have no default there: variable order is the caller's
    with pytest.raises(ValueError, match=r"\(2, 3, 4, 8, 4\)"):
        W.wind_report(x[..., :4], x[0], curve)
    with pytest.raises(ValueError):
        W.wind_report(x, x[0], curve, observation=torch.zeros(3, 2, 2, 2))
    with pytest.raises(ValueError):
        W.wind_report(x, x[0], curve, speed_grid=torch.zeros(2, 2))
    assert W.wind_fields(x[:, :0], curve, u=0, v=1)[1].shape == (2, 0, 2)


def test_unsupported_shapes_take_the_general_route(monkeypatch):
    """hw no multiple of 4, a curve of more than 256 knots, and knots that collapse in fp32: the launcher is asked, answers no, nothing
    is launched, the general route answers"""
    emu_wind_ops.install(monkeypatch, wind_ops, W)
    ref = R.reference("typical", "k61", 2, 2, 4, 25, 2, 3)
    derived, sums = W.wind_fields(torch.tensor(ref.x).view(2, 2, 4, 5, 5), _curve("k61"), u=2, v=3)
    assert R.worst_speed(derived[:, :, 0].numpy().reshape(2, 2, 25), ref)[1] and np.allclose(sums.numpy(), ref.sums, rtol=1e-6)
    xs = np.linspace(1.0, 25.0, 300)
    long_curve = W.PowerCurve(xs, R.RATED * (xs / 25.0) ** 2)
    close = W.PowerCurve([1.0, 1.0 + 2.0 ** -40, 25.0], [0.0, 1.0, R.RATED])
    ref = R.reference("typical", "k61", 2, 2, 4, 64, 2, 3)
    for curve in (long_curve, close):
        derived, sums = W.wind_fields(torch.tensor(ref.x).view(2, 2, 4, 8, 8), curve, u=2, v=3)
        want = np.interp(ref.speed, curve.speeds, curve.powers, left=0.0, right=0.0)
        assert np.allclose(derived[:, :, 1].numpy().reshape(2, 2, 64), want, rtol=1e-5, atol=1.0) and np.allclose(sums[..., 1].numpy(), want.sum(-1), rtol=1e-6)
    assert emu_wind_ops.CALLS == []  # wind_supported or the table builder said no before anything was launched
    assert not emu_wind_ops.wind_power(None, 4, 2, 3, None, 61, 1.0, None, None, None, 4, 25)
    assert not emu_wind_ops.wind_power(None, 4, 2, 3, None, 300, 1.0, None, None, None, 4, 64)


def test_a_nan_poisons_its_own_entry_only(route):
    D, T, F, H, W_ = 2, 3, 4, 8, 8
    ref = R.reference("typical", "k61", D, T, F, H * W_, 2, 3)
    curve = _curve("k61")
    X = torch.tensor(ref.x.copy()).view(D, T, F, H, W_)
    clean_d, clean_s = W.wind_fields(X, curve, u=2, v=3)
    X[0, 1, 2, 3, 3] = float("nan")   # a u
    X[1, 2, 3, 0, 0] = float("nan")   # a v
    X[1, 0, 0, 5, 5] = float("nan")   # neither: nothing happens
    X[0, 0, 1, 2, 2] = float("inf")
    derived, sums = W.wind_fields(X, curve, u=2, v=3)
    bad = torch.zeros(D, T, dtype=torch.bool)
    bad[0, 1] = bad[1, 2] = True
    assert torch.equal(torch.isnan(sums).all(dim=-1), bad) and torch.equal(torch.isnan(sums).any(dim=-1), bad)
    assert torch.equal(sums[~bad], clean_s[~bad])
    bad_cells = torch.zeros(D, T, H, W_, dtype=torch.bool)
    bad_cells[0, 1, 3, 3] = bad_cells[1, 2, 0, 0] = True
    assert torch.equal(torch.isnan(derived).all(dim=2), bad_cells) and torch.equal(torch.isnan(derived).any(dim=2), bad_cells)
    keep = ~bad_cells[:, :, None].expand_as(derived)
    assert torch.equal(derived[keep], clean_d[keep])
    assert torch.equal(torch.isnan(W.mean_power(X, curve, u=2, v=3)), bad)


# ------------------------------------------------------------------------------------------------------------------ the table

@pytest.fixture(scope="module")
def host_wind(tmp_path_factory):
    """a stand-alone program under the address and undefined-behaviour sanitizers; it is run directly, never loaded into Python.
    -ffp-contract=off: the kernel fuses no multiply with an add either (wind_core.h says so to its own compiler)."""
    return host_program.build(tmp_path_factory, "wind", sanitize=True, fp_contract_off=True, timeout=600)


BAD_CURVES = [([3.0, 3.0], [0.0, 1.0]), ([3.0, 2.0], [0.0, 1.0]), ([1.0, np.nan], [0.0, 1.0]), ([1.0, np.inf], [0.0, 1.0]), ([1.0, 2.0], [0.0, np.nan]),
              ([1.0, 2.0], [0.0, 1e39]), ([1.0, 1.0 + 2.0 ** -40, 2.0], [0.0, 1.0, 2.0]), ([1.0, 1.0 + 2.0 ** -20], [-3e38, 3e38]), ([1.0], [0.0])]


def test_the_library_s_table_is_the_python_restatement(host_wind, tmp_path):
    """c2w_wind_table (pure host code of the library), wind_core.h compiled for the host, and tests/emu_wind_ops.py: the same bytes for
    every curve, the same refusals; the bucket index puts every knot's interval within SCAN of its start, or the mode says bisect"""
    from climate2weather_amd import build as c2w_build
    c2w_build.build(verbose=False)  # no-op when libc2w_hip.so is up to date
    extra = {"tiny_span": (np.array([1.0, 1.0 + 2.0 ** -23]), np.array([0.0, 1.0])), "negative": (np.array([-2.0, 0.5, 7.0]), np.array([5.0, -1.0, 3.0]))}
    modes = {}
    for name in list(R.CURVES) + list(extra):
        xs, ps = extra[name] if name in extra else R.curve(name)
        K = xs.shape[0]
        want = emu_wind_ops.wind_table(xs, ps)
        got = wind_ops.wind_table(xs, ps)
        assert wind_ops.wind_table_bytes(K) == emu_wind_ops.wind_table_bytes(K) == want.shape[0] == 32 + 16 * (K - 1) + 512
        assert got.dtype == np.uint8 and np.array_equal(got, want), name
        xs.tofile(tmp_path / "xs"), ps.tofile(tmp_path / "ps")
        subprocess.run([str(host_wind), "table", str(K), str(tmp_path / "xs"), str(tmp_path / "ps"), str(tmp_path / "table")], check=True, timeout=600)
        assert np.array_equal(np.fromfile(tmp_path / "table", dtype=np.uint8), want), name
        xf, pf, slope, inv, mode, start = emu_wind_ops.table_parts(xs, ps)
        modes[name] = mode
        if mode == emu_wind_ops.MODE_BUCKETS:  # every fp32 speed next to a knot finds its interval within SCAN steps of its start
            s = np.concatenate([xf[:-1], np.nextafter(xf[1:], np.float32(-np.inf)), np.linspace(xf[0], xf[-1], 5000, endpoint=False).astype(np.float32)])
            s = s[(s >= xf[0]) & (s < xf[-1])]
            j = np.searchsorted(xf, s, side="right") - 1
            first = start[emu_wind_ops.bucket_of(s, xf[0], inv)].astype(np.int64)
            assert np.all(first <= j) and np.all(j - first <= emu_wind_ops.SCAN), name
    assert modes["crowded"] == emu_wind_ops.MODE_BISECT and modes["tiny_span"] == emu_wind_ops.MODE_BUCKETS
    assert all(modes[n] == emu_wind_ops.MODE_BUCKETS for n in ("k2", "k3", "k61", "tenths"))
    for xs, ps in BAD_CURVES:
        xs, ps = np.array(xs, np.float64), np.array(ps, np.float64)
        assert emu_wind_ops.wind_table(xs, ps) is None and wind_ops.wind_table(xs, ps) is None, (xs, ps)
        xs.tofile(tmp_path / "xs"), ps.tofile(tmp_path / "ps")
        assert subprocess.run([str(host_wind), "table", str(xs.shape[0]), str(tmp_path / "xs"), str(tmp_path / "ps"), str(tmp_path / "t")],
                              timeout=600).returncode == 5
    assert wind_ops.wind_table(np.linspace(1.0, 2.0, 257), np.zeros(257)) is None and wind_ops.wind_table_bytes(257) == 0 == wind_ops.wind_table_bytes(1)
    rc = _lib.load().c2w_wind_table(None, None, 2, None)
    assert rc == -1


# ------------------------------------------------------------------------------------------------------------------ the kernels' maps

@pytest.mark.parametrize("planes,F,u,v,hw", [(3, 2, 1, 0, 4), (4, 4, 2, 3, 64), (2, 3, 0, 2, 1028), (2, 4, 2, 3, 4100), (1, 4, 3, 1, 8196), (2, 2, 0, 1, 12288)])
def test_every_cell_of_the_two_planes_is_fetched_exactly_once(host_wind, tmp_path, planes, F, u, v, hw):
    """hw = 4, less than a round, one chunk + 4 cells, two chunks + 4, three whole chunks.  The fields hold their own indices, so what
    was fetched says where from; the other variables are never touched."""
    subprocess.run([str(host_wind), "visit", str(planes), str(F), str(u), str(v), str(hw), str(tmp_path / "owner")], check=True, timeout=600)
    owner = np.fromfile(tmp_path / "owner", dtype=np.int32).reshape(planes, F, hw)
    want = np.full((planes, F, hw), -1, np.int32)
    want[:, u] = want[:, v] = np.arange(planes)[:, None]
    assert np.array_equal(owner, want)


@pytest.mark.parametrize("D,T,F,u,v,hw", [(1, 1, 4, 2, 3, 4), (3, 2, 2, 1, 0, 64), (2, 1, 4, 2, 3, 4100), (1, 2, 3, 0, 2, 8196)])
def test_values_on_the_host_equal_the_emulation_bit_for_bit(host_wind, tmp_path, D, T, F, u, v, hw):
    """csrc/wind_core.h compiled for the host against tests/emu_wind_ops.py: the table, both lookups (the bucket index with its scan,
    and the bisection the crowded curve takes), the arithmetic, the accumulation order, the fold through LDS and over the chunks; every
    kind and curve, with and without the per-cell output"""
    planes = D * T
    for name in R.CURVES:
        xs, ps = R.curve(name)
        K = xs.shape[0]
        xs.tofile(tmp_path / "xs"), ps.tofile(tmp_path / "ps")
        table = torch.from_numpy(emu_wind_ops.wind_table(xs, ps).copy())
        for kind in R.KINDS:
            ref = R.reference(kind, name, D, T, F, hw, u, v)
            ref.x.tofile(tmp_path / "x")
            hub = np.float32(ref.c)
            sums = torch.full((planes, 2), -7.25, dtype=torch.float64)
            derived = torch.full((planes, 2, hw), -7.25)
            nbytes = emu_wind_ops.wind_scratch_bytes(planes, hw)
            scratch = torch.empty(nbytes // 8, dtype=torch.float64) if nbytes else None
            assert emu_wind_ops.wind_power(torch.tensor(ref.x), F, u, v, table, K, hub, sums, derived, scratch, planes, hw)
            for with_derived in (1, 0):
                subprocess.run([str(host_wind), "power", str(planes), str(F), str(u), str(v), str(hw), str(with_derived), f"{float(hub):.9g}", str(K)] +
                               [str(tmp_path / n) for n in ("xs", "ps", "x", "sums", "derived")], check=True, timeout=600)
                assert _same_bits(np.fromfile(tmp_path / "sums", dtype=np.float64).reshape(planes, 2), sums.numpy()), (name, kind, with_derived)
                if with_derived:
                    assert _same_bits(np.fromfile(tmp_path / "derived", dtype=np.float32).reshape(planes, 2, hw), derived.numpy()), (name, kind)


def test_support_predicate_scratch_and_chunking_agree():
    from climate2weather_amd import build as c2w_build
    c2w_build.build(verbose=False)
    for hw, K, want in ((4, 2, True), (16384, 256, True), (66, 8, False), (64, 257, False), (64, 1, False), (0, 8, False)):
        assert emu_wind_ops.wind_supported(hw, K) is want and wind_ops.wind_supported(hw, K) is want
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "wind_core.h")).read()
    for text in ("THREADS = 256", "MAX_K = 256", "BUCKETS = 256", "SCAN = 2", "ROUNDS = 4", "CHUNK = ROUNDS * THREADS * 4",
                 "hw >= 4 && hw % 4 == 0 && K >= 2 && K <= MAX_K", "32 + 16 * (K - 1) + 2 * BUCKETS"):
        assert text in core, text
    shared = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "ordered_sum.h")).read()
    for text in ("THREADS = 256", "GROUP = 16"):
        assert text in shared, text
    assert emu_wind_ops.CHUNK == 4096 and [emu_wind_ops.chunks(hw) for hw in (4, 4096, 4100, 16384)] == [1, 1, 2, 4]  # a function of hw alone
    for planes, hw in ((2048, 16384), (2048, 4096), (3, 4100), (1, 4), (0, 64)):
        want = planes * emu_wind_ops.chunks(hw) * 2 * 8 if emu_wind_ops.chunks(hw) > 1 and planes > 0 else 0
        assert emu_wind_ops.wind_scratch_bytes(planes, hw) == want == wind_ops.wind_scratch_bytes(planes, hw)


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_wind_supported": "int", "c2w_wind_table_bytes": "long long", "c2w_wind_table": "int", "c2w_wind_scratch_bytes": "long long",
             "c2w_wind_power": "int"}
    c_abi.assert_declared(names, "wind.hip", wind_ops, ("wind_supported", "wind_table_bytes", "wind_table", "wind_scratch_bytes", "wind_power"))
    from climate2weather_amd import ops as c2w_ops
    assert not any(hasattr(c2w_ops, fn) for fn in ("wind_supported", "wind_power"))  # ops.py's launchers are pinned by the launch replay
