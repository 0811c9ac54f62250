"""The wind-power kernels on the MI355X (csrc/wind.hip through wind_ops.wind_power and climate2weather_amd.windpower): every per-cell
speed and power and every sum against numpy.interp in float64 by the rule of tests/fp64_wind_ref.py -- the speed within 6 * 2^-24 of
itself, the power between the least and the largest value of the float64 curve over the speed's window give or take 9 * 2^-24 of the
interval's larger power, a sum within the sum of its cells' bounds -- then the properties the interface promises: the chosen interval
and the end rules exactly on speeds that are knots, the same bits wherever a plane lies in the launch, equal sums with and without the
per-cell output, nothing written past the end, nothing written for an unsupported shape, a NaN kept in its own entry.

Observed on the MI355X, worst error over the bound per kind over the five curves and the six shapes below (limit 1), per cell speed /
power, then sums speed / power: calm 0.41 / 0, 0.085 / 0; typical 0.39 / 0.25, 0.10 / 0.027; storm 0.40 / 0.18, 0.065 / 0.037; tiny
1.7e-4 / 0, 2.5e-5 / 0; huge 0 / 0 (inf meets inf); non-finite 0.40 / 0.24, 0.037 / 0.025; on_knots is judged by equality
(profiles/wind_measurements.md has the table per curve)."""
import numpy as np
import pytest
import torch

import emu_wind_ops
import fp64_kde_ref as KR
import fp64_wind_ref as R
from climate2weather_amd import wind_ops
from climate2weather_amd import windpower as W

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 64  # canary values behind each output
ONE_CHUNK_AND_FOUR = 4096 + 4
SAME_HEIGHT = dict(hub_height=10.0, reference_height=10.0)


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


_TABLES = {}


def table_of(name):
    if name not in _TABLES:
        xs, ps = R.curve(name)
        _TABLES[name] = (torch.from_numpy(wind_ops.wind_table(xs, ps).copy()).to(dev()), xs.shape[0])
    return _TABLES[name]


def power(x, u, v, curve_name, hub, with_derived=True, expect=True, K=None):
    """(sums (D, T, 2) float64, derived (D, T, 2, hw) fp32 or None) from wind_ops.wind_power on x (D, T, F, hw); the TAIL values behind
    sums, derived and the scratch must keep the canary.  expect False: the call must answer False and leave every value of the three
    buffers alone."""
    D, T, F, hw = x.shape
    planes = D * T
    table, k = table_of(curve_name)
    K = k if K is None else K
    (xd,) = to_dev(x)
    ns, nd = planes * 2, planes * 2 * hw
    nscr = wind_ops.wind_scratch_bytes(planes, hw) // 8 if expect else 1024
    sums = torch.full((ns + TAIL,), CANARY, dtype=torch.float64, device=dev())
    derived = torch.full((nd + TAIL,), CANARY, dtype=torch.float32, device=dev()) if with_derived else None
    scratch = torch.full((nscr + TAIL,), CANARY, dtype=torch.float64, device=dev())
    ok = wind_ops.wind_power(xd, F, u, v, table, K, float(np.float32(hub)), sums, derived, scratch[:nscr] if nscr else None, planes, hw)
    assert ok is expect
    assert torch.equal(sums[ns if expect else 0:], torch.full_like(sums[ns if expect else 0:], CANARY))
    assert torch.equal(scratch[nscr if expect else 0:], torch.full_like(scratch[nscr if expect else 0:], CANARY))
    if with_derived:
        assert torch.equal(derived[nd if expect else 0:], torch.full_like(derived[nd if expect else 0:], CANARY))
    return sums[:ns].view(D, T, 2), (derived[:nd].view(D, T, 2, hw) if with_derived else None)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))


# ------------------------------------------------------------------------------------------------------------------ against float64

# (D, T, F, hw, u, v): F = 2 with (1, 0) fails a swapped or wrong plane index
SHAPES = [(1, 1, 4, 4, 2, 3), (3, 2, 4, 64, 2, 3), (3, 2, 2, 64, 1, 0), (2, 3, 4, 192, 2, 3), (2, 2, 4, ONE_CHUNK_AND_FOUR, 2, 3), (2, 2, 2, ONE_CHUNK_AND_FOUR, 1, 0)]


@pytest.mark.parametrize("curve_name", R.CURVES)
def test_values_and_sums_against_float64(curve_name):
    """every field kind at every shape; the (d, t) planes differ in scale and the other variables lie near 1000, so a wrong index map
    fails.  The on_knots kind: hub factor 1 and v = 0, so the speeds are exact and the power is the kernel's arithmetic on the interval
    the definition names, bit for bit -- fp32(ps[j]) on a knot, ps[-1] at the cut-out, 0 one fp32 above it and one below the first knot."""
    worst = {}
    xs, ps = R.curve(curve_name)
    xf, pf, slope, inv, mode, start = emu_wind_ops.table_parts(xs, ps)
    for D, T, F, hw, u, v in SHAPES:
        for kind in R.KINDS:
            ref = R.reference(kind, curve_name, D, T, F, hw, u, v)
            sums, derived = power(ref.x, u, v, curve_name, ref.c)
            got, got_sums = derived.cpu().numpy(), sums.cpu().numpy()
            (rs, ok_s), (rp, ok_p) = R.worst_speed(got[:, :, 0], ref), R.worst_power(got[:, :, 1], ref)
            (rss, ok_ss), (rsp, ok_sp) = R.worst_sums(got_sums, ref)
            worst[kind] = np.maximum(worst.get(kind, np.zeros(4)), [rs, rp, rss, rsp])
            assert ok_s and ok_p and ok_ss and ok_sp, (kind, (D, T, F, hw), rs, rp, rss, rsp)
            if kind == "on_knots":
                a = np.abs(ref.x[:, :, u])
                assert np.array_equal(got[:, :, 0], a)
                s32, p32 = emu_wind_ops.cell_values32(ref.x[:, :, u], ref.x[:, :, v], 1.0, xf, pf, slope, pf[-1])
                assert same_bits(got[:, :, 1], p32)
                at_last, above, below = a == xf[-1], a == np.nextafter(xf[-1], np.float32(np.inf)), a == np.nextafter(xf[0], np.float32(-np.inf))
                assert at_last.any() and above.any() and below.any()
                assert np.all(got[:, :, 1][at_last] == pf[-1]) and np.all(got[:, :, 1][above] == 0) and np.all(got[:, :, 1][below] == 0)
                j = np.searchsorted(xf, a)
                on = xf[np.clip(j, 0, xf.shape[0] - 1)] == a
                assert on.mean() > 0.3 and np.array_equal(got[:, :, 1][on], pf[np.clip(j, 0, xf.shape[0] - 1)][on])
    print(f"{curve_name} (mode {mode}): error over bound, limit 1, speed / power / speed sums / power sums: " +
          "; ".join(f"{k} " + " / ".join(f"{x:.3g}" for x in w) for k, w in worst.items()))


# ------------------------------------------------------------------------------------------------------------------ the promises

@pytest.mark.parametrize("curve_name,hw", [("k61", 192), ("k61", ONE_CHUNK_AND_FOUR), ("crowded", 516), ("tenths", ONE_CHUNK_AND_FOUR)])
def test_same_bits_at_every_position(curve_name, hw):
    """one plane first, in the middle and last in the launch, alone, and on a second call"""
    D, T, F, u, v = 3, 2, 4, 2, 3
    ref = R.reference("typical", curve_name, D, T, F, hw, u, v)
    x = ref.x.copy()
    x[1, 1] = x[2, 1] = x[0, 0]
    a, da = power(x, u, v, curve_name, ref.c)
    b, db = power(x, u, v, curve_name, ref.c)
    assert torch.equal(a, b) and torch.equal(da, db)
    alone, dalone = power(x[:1, :1], u, v, curve_name, ref.c)
    for d, t in ((0, 0), (1, 1), (2, 1)):
        assert torch.equal(a[d, t], alone[0, 0]) and torch.equal(da[d, t], dalone[0, 0]), (d, t)
    assert not torch.equal(a[0, 1], alone[0, 0])


@pytest.mark.parametrize("curve_name,D,T,F,hw,u,v", [("k3", 2, 2, 4, 64, 2, 3), ("crowded", 1, 2, 2, ONE_CHUNK_AND_FOUR, 1, 0), ("k61", 2, 1, 4, 192, 2, 3)])
def test_sums_are_the_same_with_and_without_the_derived_fields(curve_name, D, T, F, hw, u, v):
    ref = R.reference("nonfinite", curve_name, D, T, F, hw, u, v)
    with_derived, _ = power(ref.x, u, v, curve_name, ref.c)
    without, none = power(ref.x, u, v, curve_name, ref.c, with_derived=False)
    assert none is None and same_bits(with_derived.cpu().numpy(), without.cpu().numpy())


def test_a_nan_poisons_its_own_entry_only():
    D, T, F, hw, u, v = 2, 3, 4, ONE_CHUNK_AND_FOUR, 2, 3
    ref = R.reference("typical", "k61", D, T, F, hw, u, v)
    clean, clean_d = power(ref.x, u, v, "k61", ref.c)
    x = ref.x.copy()
    x[0, 1, u, 4099] = np.nan       # in the second chunk's four cells
    x[1, 2, v, 0] = np.nan
    x[1, 0, 0, 2048] = np.nan       # neither u nor v: nothing happens
    x[0, 0, u, 7] = np.inf          # speed +inf, power 0: the speed sum is +inf, nothing is NaN
    sums, derived = power(x, u, v, "k61", ref.c)
    bad = torch.zeros(D, T, dtype=torch.bool, device=dev())
    bad[0, 1] = bad[1, 2] = True
    assert torch.equal(torch.isnan(sums).all(dim=-1), bad) and torch.equal(torch.isnan(sums).any(dim=-1), bad)
    assert float(sums[0, 0, 0]) == np.inf and float(derived[0, 0, 0, 7]) == np.inf and float(derived[0, 0, 1, 7]) == 0.0
    keep = ~bad
    keep[0, 0] = False
    assert torch.equal(sums[keep], clean[keep])
    bad_cells = torch.zeros(D, T, hw, dtype=torch.bool, device=dev())
    bad_cells[0, 1, 4099] = bad_cells[1, 2, 0] = True
    assert torch.equal(torch.isnan(derived).all(dim=2), bad_cells) and torch.equal(torch.isnan(derived).any(dim=2), bad_cells)
    same = ~bad_cells
    same[0, 0, 7] = False
    same = same[:, :, None].expand_as(derived)
    assert torch.equal(derived[same], clean_d[same])
    (X,) = to_dev(x.reshape(D, T, F, 50, 82))
    assert torch.equal(torch.isnan(W.mean_power(X, W.PowerCurve(*R.curve("k61")), u=u, v=v)), bad)


def test_unsupported_shapes_write_nothing_and_take_the_general_route():
    assert not wind_ops.wind_supported(66, 8) and not wind_ops.wind_supported(64, 257) and not wind_ops.wind_supported(64, 1)
    assert wind_ops.wind_supported(4, 2) and wind_ops.wind_supported(16384, 256)
    assert wind_ops.wind_scratch_bytes(6, 4096) == 0 and wind_ops.wind_scratch_bytes(6, ONE_CHUNK_AND_FOUR) == 6 * 2 * 2 * 8
    ref = R.reference("typical", "k61", 2, 2, 4, 66, 2, 3)
    power(ref.x, 2, 3, "k61", ref.c, expect=False)                                   # hw no multiple of 4
    power(R.reference("typical", "k61", 2, 2, 4, 64, 2, 3).x, 2, 3, "k61", ref.c, expect=False, K=257)  # K beyond the table
    (X,) = to_dev(ref.x.reshape(2, 2, 4, 6, 11))
    derived, sums = W.wind_fields(X, W.PowerCurve(*R.curve("k61")), u=2, v=3)
    assert derived.is_cuda and sums.is_cuda and derived.shape == (2, 2, 2, 6, 11) and sums.shape == (2, 2, 2)
    assert np.allclose(sums.cpu().numpy(), ref.sums, rtol=1e-13, atol=0)              # the general route: float64
    assert R.worst_speed(derived[:, :, 0].cpu().numpy().reshape(2, 2, 66), ref)[1] and R.worst_power(derived[:, :, 1].cpu().numpy().reshape(2, 2, 66), ref)[1]


def test_strided_half_precision_input_agrees_with_the_dense_route():
    base = (torch.randn(2, 3, 4, 16, 32, device=dev()) * 8.0).to(torch.float16)
    view = base[..., ::2]
    curve = W.PowerCurve(*R.curve("k61"))
    got_d, got_s = W.wind_fields(view, curve, u=2, v=3)
    dense_d, dense_s = W.wind_fields(view.float().contiguous(), curve, u=2, v=3)
    assert got_s.shape == (2, 3, 2) and torch.equal(got_s, dense_s) and torch.equal(got_d, dense_d)


# ------------------------------------------------------------------------------------------------------------------ the report

def test_report_on_the_device_equals_the_general_route():
    """(M, L, F) = (2, 3, 4) at 16 x 24 with a 4 x 6 observation, 64 grid points: the per-cell values and the sums of the device against
    the CPU general route -- float64 -- by the rule; the series are the same algebra on the sums; the densities by the KDE's own rule
    (tests/fp64_kde_ref.py) on the values the device derived"""
    M, L, F, H, W_, h, N = 2, 3, 4, 16, 24, 4, 64
    rng = np.random.default_rng(13)
    base = 6.0 * rng.standard_normal((L, F, H, W_))
    gt = (base + 2.0 * rng.standard_normal((L, F, H, W_))).astype(np.float32)
    samples = (base[None] + 2.0 * rng.standard_normal((M, L, F, H, W_))).astype(np.float32)
    obs = gt.reshape(L, F, h, H // h, 6, W_ // 6).mean(axis=(3, 5)).astype(np.float32)
    xs, ps = R.curve("k61")
    curve = W.PowerCurve(xs, ps)
    grids = dict(speed_grid=torch.linspace(0.0, 30.0, N, dtype=torch.float64), power_grid=torch.linspace(0.0, curve.rated, N, dtype=torch.float64))
    cpu = W.wind_report(torch.tensor(samples), torch.tensor(gt), curve, observation=torch.tensor(obs), **grids)
    gpu = W.wind_report(*to_dev(samples, gt), curve, observation=to_dev(obs)[0], **grids)
    assert set(gpu.keys()) == set(cpu.keys()) and all(gpu[k].is_cuda for k in gpu.keys())
    for name, x in (("sample", samples), ("gt", gt), ("obs", obs)):
        ref = R.reference_of(x.reshape(x.shape[:-2] + (-1,)), R.hub_factor(), xs, ps, 2, 3)
        lead = x.shape[:-3]
        speed, pw = gpu[f"{name}_windspeed_100"].cpu().numpy(), gpu[f"{name}_windpower"].cpu().numpy()
        assert np.allclose(cpu[f"{name}_windspeed_100"].numpy(), ref.speed.reshape(speed.shape), rtol=2 * R.EPS, atol=0)  # the CPU route is the definition
        (rs, ok_s), (rp, ok_p) = R.worst_speed(speed.reshape(lead + (-1,)), ref), R.worst_power(pw.reshape(lead + (-1,)), ref)
        mean = gpu[f"{name}_mean_power"].cpu().numpy()
        cells = x.shape[-1] * x.shape[-2]
        assert np.all((ref.s_lo / cells <= mean) & (mean <= ref.s_hi / cells))
        assert np.allclose(gpu[f"{name}_cumulative_energy"].cpu().numpy(), np.cumsum(mean / 1e3, axis=-1), rtol=1e-13, atol=0)
        assert np.allclose(mean, cpu[f"{name}_mean_power"].numpy(), rtol=1e-5)
        print(f"{name}: device against float64: error over bound (limit 1): speed {rs:.3g}, power {rp:.3g}")
        assert ok_s and ok_p
        for key, grid, vals in (("windspeed_kde", grids["speed_grid"].numpy(), speed), ("windpower_kde", grids["power_grid"].numpy(), pw)):
            got = gpu[f"{name}_{key}"].cpu().numpy().reshape(-1, N)
            for i, v in enumerate(vals.reshape((-1,) + vals.shape[-3:]) if name == "sample" else [vals]):
                v = np.ascontiguousarray(v).reshape(-1)
                hb = v.size ** -0.2 * np.std(v.astype(np.float64), ddof=1)
                f64, floor = KR.kde64(v, grid, hb)
                _, b = KR.bound(v, grid, hb, f64, floor)
                ratio, ok = KR.worst(got[i], f64, b)
                print(f"{name} {key} {i}: error over max(yardstick, floor) {ratio:.3g} (limit {KR.FACTOR})")
                assert ok
            # against the CPU report, whose densities are of ITS values: a value moved by e moves a term by about u e / h of itself, with
            # e <= 6 * 2^-24 * 40 m/s, h > 0.1 m/s and |u| < 40 that is below 1e-2 of the term in the far tails and 1e-5 where the mass is
            assert np.allclose(got.reshape(gpu[f"{name}_{key}"].shape), cpu[f"{name}_{key}"].numpy(), rtol=1e-2, atol=1e-6 * np.abs(f64).max())
        assert np.allclose(gpu[f"{name}_power_gen"].cpu().numpy(), (gpu["power_curve"] * gpu[f"{name}_windspeed_kde"]).cpu().numpy(), rtol=1e-14)
    assert torch.equal(gpu["power_curve"].cpu(), cpu["power_curve"]) and torch.equal(gpu["windspeed_range"].cpu(), cpu["windspeed_range"])
    assert set(gpu.as_dict()) == set(cpu.as_dict())
