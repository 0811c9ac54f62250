"""The CRPS kernels on the MI355X (csrc/crps.hip through ops.crps_terms and climate2weather_amd.crps): every per-cell value and every
sum against float64 by the rule of tests/fp64_crps_ref.py -- an error of at most (M + 16) 2^-24 s, s the float64 value itself for A, B
and V, A^2 for E, and their sum over the cells for a sum -- then the properties the interface promises: the same bits wherever a plane
lies in the launch, equal sums with and without the per-cell output, nothing written past the end, nothing written for an unsupported
shape, a non-finite value kept in its own entry.

Observed on the MI355X, worst error over the bound per kind over every M and shape below (limit 1), per-cell values / sums: pressure
0.38 / 0.092, pressure biased 0.38 / 0.049, temperature 0.19 / 0.080, wind 0.32 / 0.057, normalised 0.34 / 0.085, ties 0.32 / 0.14,
non-finite 0.32 / 0.049 (profiles/crps_measurements.md has the table per M)."""
import numpy as np
import pytest
import torch

import fp64_crps_ref as R
from climate2weather_amd import crps as C
from climate2weather_amd import ops

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 64  # canary values behind each output
ONE_CHUNK_AND_FOUR = 4096 + 4


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


def terms(x, y, with_cells=True, expect=True):
    """(sums (T, F, 4) float64, cells (4, T, F, hw) fp32 or None) from ops.crps_terms on x (M, T, F, hw), y (T, F, hw); the TAIL values
    behind sums, cells and the scratch must keep the canary.  expect False: the call must answer False and leave every value of the
    three buffers alone."""
    M, T, F, hw = x.shape
    xd, yd = to_dev(x, y)
    ns, ncl = T * F * 4, 4 * T * F * hw
    nd = ops.crps_scratch_bytes(T, F, hw) // 8 if expect else 1024
    sums = torch.full((ns + TAIL,), CANARY, dtype=torch.float64, device=dev())
    cells = torch.full((ncl + TAIL,), CANARY, dtype=torch.float32, device=dev()) if with_cells else None
    scratch = torch.full((nd + TAIL,), CANARY, dtype=torch.float64, device=dev())
    ok = ops.crps_terms(xd, yd, sums, cells, scratch[:nd] if nd else None, M, T, F, hw)
    assert ok is expect
    assert torch.equal(sums[ns if expect else 0:], torch.full_like(sums[ns if expect else 0:], CANARY))
    assert torch.equal(scratch[nd if expect else 0:], torch.full_like(scratch[nd if expect else 0:], CANARY))
    if with_cells:
        assert torch.equal(cells[ncl if expect else 0:], torch.full_like(cells[ncl if expect else 0:], CANARY))
    return sums[:ns].view(T, F, 4), (cells[:ncl].view(4, T, F, hw) if with_cells else None)


def same_bits(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))


# ------------------------------------------------------------------------------------------------------------------ against float64

SHAPES = [(1, 1, 4), (3, 2, 64), (2, 3, 192), (2, 2, ONE_CHUNK_AND_FOUR)]
MEMBERS = [1, 2, 3, 8, 9, 16, 17, 33, 64]  # both sides of every (K, V) boundary


@pytest.mark.parametrize("M", MEMBERS)
def test_cells_and_sums_against_float64(M):
    """every field kind at every shape; variable f differs from its neighbours in offset and scale, so a wrong index map fails"""
    worst_cells, worst_sums = {}, {}
    for T, F, hw in SHAPES:
        for kind in R.KINDS:
            x, y, cells64, sums64, s_cells, s_sums = R.reference(kind, M, T, F, hw)
            sums, cells = terms(x, y)
            rc, ok_c = R.worst(cells.cpu().numpy(), cells64, s_cells, M)
            rs, ok_s = R.worst(sums.cpu().numpy(), sums64, s_sums, M)
            worst_cells[kind], worst_sums[kind] = max(worst_cells.get(kind, 0.0), rc), max(worst_sums.get(kind, 0.0), rs)
            assert ok_c and ok_s, (kind, (T, F, hw), rc, rs)
            if kind == "ties":
                same = (x == x[:1]).all(axis=0)
                got = cells.cpu().numpy()
                assert np.all(got[1][same] == 0) and (M == 1 or np.all(got[3][same] == 0))  # identical members: B == 0, V == 0 exactly
    print(f"M {M}: error over (M + 16) 2^-24 s, limit 1: cells " + ", ".join(f"{k} {v:.3g}" for k, v in worst_cells.items()) +
          "; sums " + ", ".join(f"{k} {v:.3g}" for k, v in worst_sums.items()))


# ------------------------------------------------------------------------------------------------------------------ the promises

@pytest.mark.parametrize("M,hw", [(8, 192), (8, ONE_CHUNK_AND_FOUR), (17, 516), (64, ONE_CHUNK_AND_FOUR)])
def test_same_bits_at_every_position(M, hw):
    """one plane first, in the middle and last in the launch, alone, and on a second call"""
    T, F = 3, 2
    x, y = R.fields("temperature", M, T, F, hw)
    x, y = x.copy(), y.copy()
    x[:, 1, 1] = x[:, 2, 1] = x[:, 0, 0]
    y[1, 1] = y[2, 1] = y[0, 0]
    a, ca = terms(x, y)
    b, cb = terms(x, y)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    alone, calone = terms(x[:, :1, :1], y[:1, :1])
    for t, f in ((0, 0), (1, 1), (2, 1)):
        assert torch.equal(a[t, f], alone[0, 0]) and torch.equal(ca[:, t, f], calone[:, 0, 0]), (t, f)
    assert not torch.equal(a[0, 1], alone[0, 0])


@pytest.mark.parametrize("M,T,F,hw", [(3, 2, 2, 64), (16, 1, 2, ONE_CHUNK_AND_FOUR), (33, 2, 1, 192)])
def test_sums_are_the_same_with_and_without_the_cells(M, T, F, hw):
    x, y = R.fields("nonfinite", M, T, F, hw)
    with_cells, _ = terms(x, y)
    without, none = terms(x, y, with_cells=False)
    assert none is None and same_bits(with_cells, without)


def test_a_non_finite_value_poisons_its_own_entry_only():
    M, T, F, hw = 9, 3, 2, ONE_CHUNK_AND_FOUR
    x, y = R.fields("wind", M, T, F, hw)
    clean, clean_cells = terms(x, y)
    x, y = x.copy(), y.copy()
    x[4, 1, 0, 4099] = np.nan       # in the second chunk's four cells
    x[0, 2, 1, 0] = -np.inf
    y[0, 1, 2048] = np.inf
    sums, cells = terms(x, y)
    bad = torch.zeros(T, F, dtype=torch.bool, device=dev())
    bad[1, 0] = bad[2, 1] = bad[0, 1] = True
    assert torch.equal(torch.isnan(sums).all(dim=-1), bad) and torch.equal(torch.isnan(sums).any(dim=-1), bad)
    assert torch.equal(sums[~bad], clean[~bad])
    bad_cells = torch.zeros(T, F, hw, dtype=torch.bool, device=dev())
    bad_cells[1, 0, 4099] = bad_cells[2, 1, 0] = bad_cells[0, 1, 2048] = True
    assert torch.equal(torch.isnan(cells).all(dim=0), bad_cells) and torch.equal(torch.isnan(cells).any(dim=0), bad_cells)
    assert torch.equal(cells[:, ~bad_cells], clean_cells[:, ~bad_cells])
    got = C.crps(*to_dev(x.reshape(M, T, F, 50, 82), y.reshape(T, F, 50, 82)))
    assert torch.equal(torch.isnan(got), bad)


def test_unsupported_shapes_write_nothing_and_take_the_general_route():
    assert not ops.crps_supported(66, 8) and not ops.crps_supported(64, 65) and not ops.crps_supported(64, 0)
    assert ops.crps_supported(4, 1) and ops.crps_supported(16384, 64)
    assert ops.crps_scratch_bytes(3, 2, 4096) == 0 and ops.crps_scratch_bytes(3, 2, ONE_CHUNK_AND_FOUR) == 3 * 2 * 2 * 4 * 8
    for M, H, W_ in ((8, 6, 11), (65, 8, 8)):
        hw = H * W_
        x, y = R.fields("temperature", M, 2, 2, hw)
        terms(x, y, expect=False)
        S, Tr = to_dev(x.reshape(M, 2, 2, H, W_), y.reshape(2, 2, H, W_))
        sums, cells = C.ensemble_terms(S, Tr, cells=True)
        assert sums.is_cuda and cells.is_cuda and sums.shape == (2, 2, 4) and cells.shape == (4, 2, 2, H, W_)
        cells64 = R.terms64(x, y)
        assert np.allclose(sums.cpu().numpy(), np.moveaxis(cells64.sum(-1), 0, -1), rtol=1e-13, atol=0)  # the general route: float64
        assert R.worst(cells.cpu().numpy().reshape(cells64.shape), cells64, R.yardsticks(cells64), M)[1]
        want = R.scores64(sums.cpu().numpy(), M, hw)
        assert np.allclose(C.crps(S, Tr).cpu().numpy(), want["crps"], rtol=1e-13, atol=0)
        assert np.allclose(C.spread_skill(S, Tr)[2].cpu().numpy(), want["ratio"], rtol=1e-13, atol=0)


def test_strided_half_precision_input_agrees_with_the_dense_route():
    base = (torch.randn(5, 3, 2, 16, 32, device=dev()) * 3.0 + 1.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]
    got, got_cells = C.ensemble_terms(view, truth, cells=True)
    dense, dense_cells = C.ensemble_terms(view.float().contiguous(), truth.float().contiguous(), cells=True)
    assert got.shape == (3, 2, 4) and torch.equal(got, dense) and torch.equal(got_cells, dense_cells)


# ------------------------------------------------------------------------------------------------------------------ the report

def test_report_on_the_device_equals_the_cpu_general_route():
    """(M, T, F) = (8, 5, 2) at 16 x 24, de-normalised (temperature-like and pressure-like): the device sums against the CPU general
    route -- float64 -- by the rule; the report's scores are the same algebra on those sums"""
    M, T, F, H, W_ = 8, 5, 2, 16, 24
    rng = np.random.default_rng(9)
    off, sd = np.array([280.0, 101325.0]), np.array([10.0, 1200.0])
    centre = off[None, :, None, None] + sd[None, :, None, None] * rng.standard_normal((T, F, H, W_))
    truth = (centre + 0.01 * sd[None, :, None, None] * rng.standard_normal((T, F, H, W_))).astype(np.float32)
    samples = (centre[None] + 0.012 * sd[None, None, :, None, None] * rng.standard_normal((M, T, F, H, W_))).astype(np.float32)
    cpu_sums, cpu_cells = C.ensemble_terms(torch.tensor(samples), torch.tensor(truth), cells=True)
    S, Tr = to_dev(samples, truth)
    gpu_sums = C.ensemble_terms(S, Tr)
    s_cells = R.yardsticks(cpu_cells.double().numpy().reshape(4, T, F, -1))
    cells64 = R.terms64(samples.reshape(M, T, F, -1), truth.reshape(T, F, -1))
    assert np.allclose(cpu_sums.numpy(), np.moveaxis(cells64.sum(-1), 0, -1), rtol=1e-12, atol=0)  # the CPU route is the definition
    ratio, ok = R.worst(gpu_sums.cpu().numpy(), cpu_sums.numpy(), np.moveaxis(R.yardsticks(cells64).sum(-1), 0, -1), M)
    print(f"device sums against the CPU general route: error over the bound {ratio:.3g} (limit 1)")
    assert ok and s_cells.shape == cells64.shape
    cpu = C.crps_report(torch.tensor(samples), torch.tensor(truth), names=["tas", "psl"])
    gpu = C.crps_report(S, Tr, names=["tas", "psl"])
    want = R.scores64(gpu_sums.cpu().numpy(), M, H * W_)
    tot = gpu_sums.cpu().numpy().sum(axis=0)
    # what the rule for the sums allows a derived score, to first order: crps is linear in the sums of A and B; a square root halves a
    # relative error; the ratio takes both
    s_tot, n, fac = R.yardsticks(cells64).sum(axis=(1, 3)), T * H * W_, 1.01 * R.factor(M)  # (4, F)
    e_tot = cells64[2].sum(axis=(0, 2))
    allow = dict(crps=fac * (s_tot[0] + s_tot[1] / M ** 2) / n, rmse=None, spread=None, ratio=None)
    rel = dict(rmse=0.5 * fac * s_tot[2] / e_tot, spread=0.5 * fac * np.ones(F))
    rel["ratio"] = rel["rmse"] + rel["spread"]
    for f, (name, v) in enumerate(gpu):
        assert all(t.is_cuda and t.dtype == torch.float64 for t in v.values())
        assert np.allclose(v["crps_by_time"].cpu().numpy(), want["crps"][:, f], rtol=1e-13, atol=0)
        assert float(v["crps"]) == pytest.approx((tot[f, 0] - tot[f, 1] / M ** 2) / n, rel=1e-13)
        assert abs(float(v["crps"]) - float(cpu[name]["crps"])) <= allow["crps"][f]
        for key in ("rmse", "spread", "ratio"):
            assert float(v[key]) == pytest.approx(want[key][f], rel=1e-13)
            assert abs(float(v[key]) - float(cpu[name][key])) <= rel[key][f] * float(cpu[name][key]), key
    assert set(gpu.as_dict()) == set(cpu.as_dict())
