"""CPU checks of the ensemble SSIM (climate2weather_amd.ssim): both routes of ssim.ssim -- the general float64 avg_pool2d one and the
launcher's, with tests/emu_ssim_ops.py standing in for the HIP kernel -- against the float64 definition, the report against a
line-by-line restatement of the reference's loop, the argument checks, the rule's negative control, the kernel's own arithmetic compiled
for the host (csrc/ssim_core.h), and the C declarations against the ctypes prototypes."""
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_ssim_ops
import fp64_ssim_ref as R
import host_program
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd import ssim as ssim_mod

# Both CPU routes are float64 end to end on the fp32 numbers the reference sees.  The straight u_xx - u_x^2 loses offset^2 / variance
# of float64's 1.1e-16 -- 1e10 / 9e4 on the pressure-like pair's noise -- times a few tens of operations: 1e-10 at the worst.
ROUTE_TOL = 1e-9


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of ssim.ssim on CPU tensors"""
    if request.param == "launcher":
        emu_ssim_ops.install(monkeypatch, c2w_ops, ssim_mod)
    return request.param


# ------------------------------------------------------------------------------------------------------------------ both routes

@pytest.mark.parametrize("H,W,win", [(16, 16, 15), (16, 16, 7), (24, 40, 15), (32, 32, 11)])
def test_every_field_kind_against_float64(route, H, W, win):
    kinds, x, y, rng, S64, _ = R.cases(H, W, win)
    got = ssim_mod.ssim(torch.tensor(x), torch.tensor(y), data_range=torch.tensor(rng), win_size=win)
    assert got.dtype == torch.float64 and got.shape == (len(kinds),)
    err = np.abs(got.numpy() - S64)
    print(f"{route} {H}x{W} win {win}: " + ", ".join(f"{k} {e:.1e}" for k, e in zip(kinds, err)))
    assert np.all(err <= ROUTE_TOL)
    assert S64[kinds.index("anti")] < 0
    assert abs(got[kinds.index("identical")].item() - 1.0) <= R.FACTOR * R.FLOOR


@pytest.mark.parametrize("H,W,win", [(20, 20, 9), (15, 33, 5), (256, 256, 15)])
def test_general_route_takes_what_the_kernel_does_not(H, W, win):
    p = R.pairs(H, W)
    x, y = p["temperature"]
    rng = R.pair_range(x, y)
    got = ssim_mod.ssim(torch.tensor(x), torch.tensor(y), data_range=rng, win_size=win)
    assert got.shape == () and abs(got.item() - R.ssim64(x, y, rng, win)) <= ROUTE_TOL


def test_unsupported_shapes_ask_the_launcher_once_and_take_the_general_route(monkeypatch):
    emu_ssim_ops.install(monkeypatch, c2w_ops, ssim_mod)
    ssim_mod.ssim(torch.randn(3, 2, 16, 24), torch.randn(2, 16, 24), win_size=7)
    x, y = torch.randn(2, 20, 20), torch.randn(20, 20)
    got = ssim_mod.ssim(x, y, data_range=4.0, win_size=9)  # asked, answered "unsupported", general route taken
    assert emu_ssim_ops.CALLS == [(6, 2, 16, 24, 7), (2, 1, 20, 20, 9)]
    for i in range(2):
        assert abs(got[i].item() - R.ssim64(x[i].numpy(), y.numpy(), 4.0, 9)) <= ROUTE_TOL


def test_pairing_rule_and_per_slot_ranges(route):
    """samples (M, T, F) against truth (T, F): pair i meets truth i % (T F) and the range of that slot"""
    rng = np.random.default_rng(3)
    truth = rng.standard_normal((3, 2, 16, 16)).astype(np.float32)
    samples = (truth[None] + 0.5 * rng.standard_normal((2, 3, 2, 16, 16))).astype(np.float32)
    ranges = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=np.float32)
    got = ssim_mod.ssim(torch.tensor(samples), torch.tensor(truth), data_range=torch.tensor(ranges), win_size=7).numpy()
    assert got.shape == (2, 3, 2)
    for m in range(2):
        for t in range(3):
            for f in range(2):
                assert abs(got[m, t, f] - R.ssim64(samples[m, t, f], truth[t, f], float(ranges[t, f]), 7)) <= ROUTE_TOL


def test_default_range_is_the_reference_s_per_variable(route):
    rng = np.random.default_rng(4)
    truth = rng.standard_normal((3, 2, 16, 16)).astype(np.float32) * np.array([1.0, 50.0], dtype=np.float32)[None, :, None, None]
    samples = (truth[None] * 1.1).astype(np.float32)
    got = ssim_mod.ssim(torch.tensor(samples), torch.tensor(truth), win_size=7).numpy()
    for f in range(2):
        values, _, _ = R.ssim_reference(samples[:, :, f], truth[:, f], win=7)
        assert np.abs(got[:, :, f] - values).max() <= ROUTE_TOL
    one = ssim_mod.ssim(torch.tensor(samples[:, :, 0]), torch.tensor(truth[:, 0]), win_size=7).numpy()  # (M, T, H, W): one variable
    assert np.abs(one - R.ssim_reference(samples[:, :, 0], truth[:, 0], win=7)[0]).max() <= ROUTE_TOL


def test_any_dtype_any_strides_and_the_empty_batch(route):
    base = torch.randn(3, 2, 16, 32, dtype=torch.float64)
    view, tv = base[..., ::2], base[0, :, :, 1::2]  # (3, 2, 16, 16) and (2, 16, 16), strided
    got = ssim_mod.ssim(view, tv, data_range=3.0, win_size=11)
    assert got.shape == (3, 2) and got.dtype == torch.float64
    x32, y32 = view.float().numpy(), tv.float().numpy()
    for i in range(3):
        for f in range(2):
            assert abs(got[i, f].item() - R.ssim64(x32[i, f], y32[f], 3.0, 11)) <= ROUTE_TOL
    half = ssim_mod.ssim(view.to(torch.float16), tv.to(torch.float16), data_range=3.0, win_size=11)
    xh, yh = view.to(torch.float16).double().numpy(), tv.to(torch.float16).double().numpy()
    assert half.dtype == torch.float64 and abs(half[2, 1].item() - R.ssim64(xh[2, 1], yh[1], 3.0, 11)) <= ROUTE_TOL
    off = torch.randn(2 * 16 * 16 + 1)[1:].view(2, 16, 16)  # 4-byte aligned only
    assert abs(ssim_mod.ssim(off, off[0], data_range=2.0, win_size=7)[0].item() - 1.0) <= ROUTE_TOL
    empty = ssim_mod.ssim(torch.zeros(0, 2, 16, 16), torch.zeros(2, 16, 16))
    assert empty.shape == (0, 2) and empty.dtype == torch.float64


def test_argument_checks():
    x, y = torch.zeros(2, 16, 24), torch.zeros(16, 24)
    for win in (8, 17, 1, 25):  # even; wider than H; no sample covariance; wider than both
        with pytest.raises(ValueError):
            ssim_mod.ssim(x, y, win_size=win)
    with pytest.raises(ValueError):
        ssim_mod.ssim(x, torch.zeros(16, 16))
    with pytest.raises(ValueError):
        ssim_mod.ssim(y, x)
    with pytest.raises(ValueError):
        ssim_mod.ssim(torch.zeros(16), torch.zeros(16))


def test_nan_pair_gives_nan_and_spares_its_neighbours(route):
    x, y = torch.randn(2, 2, 16, 16), torch.randn(2, 16, 16)
    x[0, 1, 4, 4] = float("nan")  # pair 1 of the flat batch
    S = ssim_mod.ssim(x, y, data_range=6.0, win_size=7).reshape(-1)
    assert torch.isnan(S[1]) and torch.isfinite(S[[0, 2, 3]]).all()
    y[1, 8, 8] = float("nan")  # truth slot 1 meets pairs 1 and 3
    S = ssim_mod.ssim(x, y, data_range=6.0, win_size=7).reshape(-1)
    assert torch.isnan(S[[1, 3]]).all() and torch.isfinite(S[[0, 2]]).all()


# ------------------------------------------------------------------------------------------------------------------ report

def _ensemble(H, W, M=2, T=3, F=2, seed=5):
    """de-normalised: variable 0 temperature-like, variable 1 pressure-like"""
    rng = np.random.default_rng(seed)
    off, sd = np.array([280.0, 101325.0]), np.array([10.0, 1200.0])
    truth = np.stack([np.stack([off[f] + sd[f] * R.smooth(H, W, 50 + 10 * t + f) for f in range(F)]) for t in range(T)])
    samples = truth[None] + 0.3 * sd[None, None, :, None, None] * rng.standard_normal((M, T, F, H, W))
    return samples.astype(np.float32), truth.astype(np.float32)


@pytest.mark.parametrize("H,W", [(16, 16), (24, 40)])
def test_report_against_the_reference_loop(route, H, W):
    samples, truth = _ensemble(H, W)
    rep = ssim_mod.ssim_report(torch.tensor(samples), torch.tensor(truth), names=["tas", "psl"])
    assert rep.names == ["tas", "psl"]
    for f, (name, v) in enumerate(rep):
        values, mean, data_range = R.ssim_reference(samples[:, :, f], truth[:, f])
        assert set(v) == {"ssim_over_time", "ssim", "data_range"} and rep[name] is v
        assert v["ssim_over_time"].shape == (2, 3) and v["ssim"].shape == (2,) and v["ssim"].dtype == torch.float64
        assert float(v["data_range"]) == pytest.approx(data_range, rel=1e-6)
        assert np.abs(v["ssim_over_time"].numpy() - values).max() <= ROUTE_TOL
        assert np.abs(v["ssim"].numpy() - mean).max() <= ROUTE_TOL
    flat = rep.as_dict()
    assert set(flat) == {f"ssim/{n}/ssim{s}" for n in ("tas", "psl") for s in ("", "_std")}
    assert all(isinstance(x, float) for x in flat.values())
    mean1 = R.ssim_reference(samples[:, :, 1], truth[:, 1])[1]
    assert flat["ssim/psl/ssim"] == pytest.approx(mean1.mean(), abs=ROUTE_TOL) and flat["ssim/psl/ssim_std"] == pytest.approx(mean1.std(), abs=ROUTE_TOL)


def test_report_t_step_names_and_argument_checks(route):
    samples, truth = _ensemble(16, 16, T=5)
    rep = ssim_mod.ssim_report(torch.tensor(samples), torch.tensor(truth), t_step=2, win_size=7)
    assert rep.names == ["var0", "var1"] and set(rep.as_dict("eval")) == {f"eval/var{f}/ssim{s}" for f in range(2) for s in ("", "_std")}
    for f, (_, v) in enumerate(rep):
        values, mean, _ = R.ssim_reference(samples[:, ::2, f], truth[::2, f], win=7)  # the range too is over the kept frames only
        assert v["ssim_over_time"].shape == (2, 3)
        assert np.abs(v["ssim_over_time"].numpy() - values).max() <= ROUTE_TOL and np.abs(v["ssim"].numpy() - mean).max() <= ROUTE_TOL
    with pytest.raises(ValueError):
        ssim_mod.ssim_report(torch.tensor(samples), torch.tensor(truth[:2]))
    with pytest.raises(ValueError):
        ssim_mod.ssim_report(torch.tensor(samples), torch.tensor(truth), names=["only_one"])
    with pytest.raises(ValueError):
        ssim_mod.ssim_report(torch.tensor(samples), torch.tensor(truth), t_step=0)


# ------------------------------------------------------------------------------------------------------------------ the rule bites

def test_an_unpivoted_fp32_port_fails_the_rule_on_the_pressure_like_pair():
    kinds, x, y, rng, S64, b = R.cases(16, 16, 15)
    i = kinds.index("pressure")
    e = abs(R.ssim_straight32(x[i], y[i], float(rng[i]), 15) - S64[i])
    print(f"pressure-like 16x16: straight fp32 error {e:.3g}, bound {b[i]:.3g}")
    assert e > b[i]
    j = kinds.index("white")  # and it is the offset that does it: on unit-scale noise the same port passes
    assert abs(R.ssim_straight32(x[j], y[j], float(rng[j]), 15) - S64[j]) <= b[j]


# ------------------------------------------------------------------------------------------------------------------ the kernel's arithmetic

@pytest.fixture(scope="module")
def host_ssim(tmp_path_factory):
    return host_program.build(tmp_path_factory, "ssim", sanitize=False, timeout=300)


def _run_host(exe, tmp_path, x, y, rng, win):
    n, nt, (H, W) = len(x), len(y), x.shape[-2:]
    np.ascontiguousarray(x).tofile(tmp_path / "x.f32"), np.ascontiguousarray(y).tofile(tmp_path / "y.f32"), np.ascontiguousarray(rng).tofile(tmp_path / "r.f32")
    subprocess.run([str(exe), str(H), str(W), str(win), str(n), str(nt), str(tmp_path / "x.f32"), str(tmp_path / "y.f32"), str(tmp_path / "r.f32"),
                    str(tmp_path / "out.f64")], check=True, timeout=120)
    return np.fromfile(tmp_path / "out.f64", dtype=np.float64)


@pytest.mark.parametrize("H,W,win", [(16, 16, 15), (24, 40, 15), (32, 32, 15), (128, 128, 15), (16, 16, 7), (16, 16, 11)])
def test_kernel_phases_on_the_host_meet_the_rule(host_ssim, tmp_path, H, W, win):
    """csrc/ssim_core.h compiled for the host, its phases run one thread after the other: every index map of the kernel (slots, the ring,
    the strips, the shared middle of four sums, the partials' order) and its fp32 arithmetic, against float64 by the rule of the GPU tier."""
    kinds, x, y, rng, S64, b = R.cases(H, W, win)
    S = _run_host(host_ssim, tmp_path, x, y, rng, win)
    for i, k in enumerate(kinds):
        e = abs(S[i] - S64[i])
        print(f"{H}x{W} win {win} {k}: error {e:.3g} bound {b[i]:.3g} ratio to max(yardstick, floor) {e / (b[i] / R.FACTOR):.3g}")
        assert e <= b[i], (k, e, b[i])
    assert abs(S[kinds.index("identical")] - 1.0) <= R.FACTOR * R.FLOOR


def test_kernel_phases_on_the_host_pairing_and_slots(host_ssim, tmp_path):
    """5 pairs against 2 truth fields at 16 x 24 (four pairs a workgroup, the second one partly empty): i % n_truth, the slot's own
    range, and the same bits for the same pair in another slot"""
    rng = np.random.default_rng(8)
    y = rng.standard_normal((2, 16, 24)).astype(np.float32)
    x = (y[np.arange(5) % 2] + 0.4 * rng.standard_normal((5, 16, 24))).astype(np.float32)
    x[4] = x[0]  # pair 4 = pair 0: slot 0 of the second workgroup against slot 0 of the first
    ranges = np.array([5.0, 9.0], dtype=np.float32)
    S = _run_host(host_ssim, tmp_path, x, y, ranges, 7)
    for i in range(5):
        S64 = R.ssim64(x[i], y[i % 2], float(ranges[i % 2]), 7)
        assert abs(S[i] - S64) <= R.bound(x[i], y[i % 2], float(ranges[i % 2]), 7, S64)
    assert S[4] == S[0]
    x[2] = x[0]  # slot 2 of the first workgroup
    assert _run_host(host_ssim, tmp_path, x, y, ranges, 7)[2] == S[0]


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_ssim_supported": "int", "c2w_ssim": "int"}
    c_abi.assert_declared(names, "ssim.hip")

