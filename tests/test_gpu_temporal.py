"""The temporal-increment kernel on the MI355X (csrc/temporal.hip through temporal_ops and climate2weather_amd.temporal): every entry
of the table against float64 by the rules of tests/fp64_temporal_ref.py -- A1 within 2 * 2^-24 and A2 within 3 * 2^-24 of themselves,
E2 within 6 * 2^-24 sum (|dx| + |dy|)^2, each plus one fp32 denormal per cell -- then the properties the interface promises: the same
bits wherever a plane series lies in the launch, nothing written past the end, nothing written for an unsupported shape, a non-finite
value kept in its own entries, the same table on another stream, and the public functions on the device against the general float64
route.

profiles/temporal_measurements.md has the observed worst fraction of each rule per kind."""
import numpy as np
import pytest
import torch

import fp64_temporal_ref as R
from climate2weather_amd import temporal as TP
from climate2weather_amd import temporal_ops

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 64  # canary values behind each output
MAX_L = 24


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [None if a is None else torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


def terms(x, y, L, expect=True):
    """S (D, T, F, L, 3) float64 from temporal_ops.tincr_terms on x (n_rep, T, F, hw), y (T, F, hw) or None; the TAIL values behind S and
    the scratch must keep the canary.  expect False: the call must answer False and leave every value of both buffers alone."""
    n_rep, T, F, hw = x.shape
    xd, yd = to_dev(x, y)
    D = n_rep + (y is not None)
    n = D * T * F * L * 3
    nd = temporal_ops.tincr_scratch_bytes(D, T, F, hw, L) // 8 if expect else 1024
    S = torch.full((n + TAIL,), CANARY, dtype=torch.float64, device=dev())
    scratch = torch.full((nd + TAIL,), CANARY, dtype=torch.float64, device=dev())
    ok = temporal_ops.tincr_terms(xd, yd, S, scratch[:nd] if nd else None, n_rep, T, F, hw, L)
    assert ok is expect
    assert torch.equal(S[n if expect else 0:], torch.full_like(S[n if expect else 0:], CANARY))
    assert torch.equal(scratch[nd if expect else 0:], torch.full_like(scratch[nd if expect else 0:], CANARY))
    return S[:n].view(D, T, F, L, 3)


# ------------------------------------------------------------------------------------------------------------------ against float64

@pytest.mark.parametrize("hw", [4, 4096, 4100, 16384])
def test_the_table_against_float64(hw):
    """T in {1, 2, 7}, L in {1, 8, 9, 24} (L >= T included; 9 is no multiple of a fold pass, 24 the maximum), n_rep in {1, 3}, with and
    without a truth; the field kinds take turns, so every kind meets every shape.  Variable f differs from its neighbours in offset
    and scale, so a wrong index map fails."""
    worst, k = {}, 0
    for T in (1, 2, 7):
        for n_rep in (1, 3):
            for with_truth in (True, False):
                for L in (1, 8, 9, 24):
                    kind = R.KINDS[k % len(R.KINDS)]
                    k += 1
                    x, y, S, Y = R.reference(kind, n_rep, T, 2, hw, MAX_L, with_truth)  # the table at L is the first L lags of it
                    got = terms(x, y, L)
                    r, ok = R.worst_table(got.cpu().numpy(), S[:, :, :, :L], Y[:, :, :, :L], hw)
                    worst[kind] = np.maximum(worst.get(kind, np.zeros(3)), r)
                    assert ok, (kind, (n_rep, with_truth, T, hw, L), r)
    print(f"hw {hw}: error over the rules (A1, A2, E2), limit 1: " + ", ".join(f"{k_} {v[0]:.3g} {v[1]:.3g} {v[2]:.3g}" for k_, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------ the promises

@pytest.mark.parametrize("hw,L", [(64, 3), (4100, 9), (16384, 24)])
def test_the_same_series_gives_the_same_bits_at_every_position(hw, L):
    """one series of planes as the truth, as the first and as the last data set, in the first and in the last variable, alone, and on
    a second call"""
    n_rep, T, F = 3, 5, 3
    x, y = R.fields("temperature", n_rep, T, F, hw)
    x, y = x.copy(), y.copy()
    series = x[1, :, 1].copy()
    x[0, :, 0] = x[2, :, 2] = y[:, 2] = series
    a, b = terms(x, y, L), terms(x, y, L)
    assert torch.equal(a, b)
    alone = terms(series[None, :, None], None, L)[0, :, 0]  # (T, L, 3)
    for d, f in ((2, 1), (1, 0), (3, 2), (0, 2)):
        assert torch.equal(a[d, :, f, :, :2], alone[..., :2]), (d, f)
    assert torch.equal(a[3, :, 2, :, 2], torch.zeros_like(a[3, :, 2, :, 2]))  # the truth's own series as a member: no tendency error
    assert not torch.equal(a[1, :, 1, :, :2], alone[..., :2])
    moved = terms(x[::-1].copy(), y, L)  # the data sets in reverse order: every row keeps all its bits
    assert torch.equal(moved[1:], a[1:].flip(0)) and torch.equal(moved[0], a[0])


def test_a_non_finite_value_poisons_its_own_entries_only():
    n_rep, T, F, hw, L = 3, 8, 2, 4100, 3
    x, y = R.fields("wind", n_rep, T, F, hw)
    clean = terms(x, y, L)
    x, y = x.copy(), y.copy()
    x[1, 4, 0, 4099] = np.nan    # the last cell: the second chunk
    x[2, 7, 1, 0] = -np.inf      # the last hour: backward only
    y[1, 1, 2048] = np.inf       # the truth: column 2 of every row
    S = terms(x, y, L)
    bad = torch.zeros(n_rep + 1, T, F, L, 3, dtype=torch.bool, device=dev())
    for d, t, f in ((2, 4, 0), (3, 7, 1), (0, 1, 1)):
        for tau in range(1, L + 1):
            for anchor in (t, t - tau):
                if 0 <= anchor and anchor + tau < T:
                    bad[d, anchor, f, tau - 1] = True
                    if d == 0:
                        bad[:, anchor, f, tau - 1, 2] = True
    assert torch.equal(torch.isnan(S), bad) and torch.equal(S[~bad], clean[~bad])
    Sx, Sy = to_dev(x.reshape(n_rep, T, F, 41, 100), y.reshape(T, F, 41, 100))
    assert torch.equal(torch.isnan(TP.increment_terms(Sx, Sy, L)), bad)
    assert torch.equal(torch.isnan(TP.tendency_rmse(Sx, Sy, L)), bad[1:, ..., 2].any(dim=1))


def test_strided_half_precision_input_agrees_with_the_dense_route():
    base = (torch.randn(3, 6, 2, 16, 64, device=dev()) * 3.0 + 1.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]
    dense, dtruth = view.float().contiguous(), truth.float().contiguous()
    assert torch.equal(TP.increment_terms(view, truth, 4), TP.increment_terms(dense, dtruth, 4))
    assert torch.equal(TP.increment_terms(view, None, 4), TP.increment_terms(dense, None, 4))


def test_unsupported_shapes_write_nothing_and_take_the_general_route():
    assert not temporal_ops.tincr_supported(6, 6) and not temporal_ops.tincr_supported(64, 25) and not temporal_ops.tincr_supported(64, 0)
    assert temporal_ops.tincr_supported(4, 1) and temporal_ops.tincr_supported(16384, 24)
    assert temporal_ops.tincr_scratch_bytes(4, 7, 2, 4096, 6) == 0 and temporal_ops.tincr_scratch_bytes(4, 7, 2, 4100, 6) == 4 * 7 * 2 * 2 * 18 * 8
    for H, W_, L in ((2, 3, 6), (4, 4, 25)):  # hw = 6; L = 25
        x, y = R.fields("temperature", 2, 30, 2, H * W_)
        terms(x, y, L, expect=False)
        got = TP.increment_terms(*to_dev(x.reshape(2, 30, 2, H, W_), y.reshape(30, 2, H, W_)), max_lag=L)
        want, _ = R.table64(x, y, L)
        assert got.is_cuda and np.allclose(got.cpu().numpy(), want, rtol=1e-13, atol=0)  # the general route: float64


def test_a_call_on_another_stream_gives_the_same_table():
    x, y = R.fields("pressure", 3, 7, 2, 4100)
    xd, yd = to_dev(x.reshape(3, 7, 2, 41, 100), y.reshape(7, 2, 41, 100))
    want = TP.increment_terms(xd, yd, 9)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = TP.increment_terms(xd, yd, 9)
    side.synchronize()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------------ the public functions

def test_public_functions_on_the_device_equal_the_cpu_general_route():
    """(M, T, F) = (4, 13, 2) at 16 x 24, de-normalised (temperature-like and pressure-like series): the table of the device against the
    CPU general route -- float64 -- by the rules; the scores and the report are the same algebra on the table"""
    M, T, F, H, W_, L = 4, 13, 2, 16, 24, 6
    hw = H * W_
    xt, yt = R.fields("temperature", M, T, 1, hw)
    xp, yp = R.fields("pressure", M, T, 1, hw)
    samples, truth = np.concatenate([xt, xp], axis=2).reshape(M, T, F, H, W_), np.concatenate([yt, yp], axis=1).reshape(T, F, H, W_)
    Sc, Tc = torch.tensor(samples), torch.tensor(truth)
    S_, Tr = to_dev(samples, truth)
    cpu, gpu = TP.increment_terms(Sc, Tc, L), TP.increment_terms(S_, Tr, L)
    want, Y = R.table64(samples.reshape(M, T, F, hw), truth.reshape(T, F, hw), L)
    assert np.allclose(cpu.numpy(), want, rtol=1e-12, atol=0)  # the CPU route is the definition
    r, ok = R.worst_table(gpu.cpu().numpy(), cpu.numpy(), Y, hw)
    print(f"device table against the CPU general route: error over the rules (A1, A2, E2), limit 1: {r[0]:.3g} {r[1]:.3g} {r[2]:.3g}")
    assert gpu.is_cuda and ok
    # a pooled value is a sum of entries over a count: the rules carry over; a square root halves a relative error
    pooled_y = Y.sum(axis=1) / (np.array([T - tau for tau in range(1, L + 1)]) * hw)  # (D, F, L)
    for got, ref in zip(TP.structure_functions(S_, Tr, L), TP.structure_functions(Sc, Tc, L)):
        assert got.is_cuda and got.dtype == torch.float64 and np.all(np.abs(got.cpu().numpy() - ref.numpy()) <= 1.01 * R.A2_C * R.EPS * ref.numpy())
    for order in (1, 2):
        got, ref = TP.variability_ratio(S_, Tr, L, order=order), TP.variability_ratio(Sc, Tc, L, order=order)
        assert got.is_cuda and np.all(np.abs(got.cpu().numpy() - ref.numpy()) <= 1.01 * 2 * R.A2_C * R.EPS * ref.numpy())
    got, ref = TP.tendency_rmse(S_, Tr, L), TP.tendency_rmse(Sc, Tc, L)
    allow = 1.01 * 0.5 * R.E2_C * R.EPS * pooled_y[1:] / ref.numpy()  # d sqrt(v) = dv / (2 sqrt(v))
    assert got.is_cuda and np.all(np.abs(got.cpu().numpy() - ref.numpy()) <= allow)
    rc, rg = TP.temporal_report(Sc, Tc, names=["tas", "psl"], max_lag=L, period=6), TP.temporal_report(S_, Tr, names=["tas", "psl"], max_lag=L, period=6)
    for name, v in rg:
        assert all(t.is_cuda and t.dtype == torch.float64 for t in v.values())
        for key in ("ratio_1", "ratio_2", "tendency_rmse", "structure_2_truth"):
            assert torch.allclose(v[key].cpu(), rc[name][key], rtol=1e-5, atol=0), (name, key)
        assert torch.equal(v["phase_count"].cpu(), rc[name]["phase_count"])
    assert set(rg.as_dict()) == set(rc.as_dict())
