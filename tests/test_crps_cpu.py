"""CPU checks of the ensemble CRPS and spread-skill (climate2weather_amd.crps): the definition itself against the integral form
evaluated exactly in float64, both routes of every public function -- the general float64 one and the launcher's, with
tests/emu_crps_ops.py standing in for the HIP kernels -- against the float64 definition by the rule of tests/fp64_crps_ref.py, the
rule's negative control (a straight fp32 port fails it), the report, the argument checks, the kernels' own index maps and arithmetic
compiled for the host (csrc/crps_core.h) under the address and undefined-behaviour sanitizers, and the C declarations against the
ctypes prototypes."""
import os
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_crps_ops
import fp64_crps_ref as R
import host_program
from climate2weather_amd import crps as C
from climate2weather_amd import ops as c2w_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of crps.ensemble_terms on CPU tensors"""
    if request.param == "launcher":
        emu_crps_ops.install(monkeypatch, c2w_ops, C)
    return request.param


def _t5(x, y, H, W_):
    """(M, T, F, hw), (T, F, hw) arrays -> the (M, T, F, H, W), (T, F, H, W) tensors of the public interface"""
    return torch.tensor(x).view(x.shape[:3] + (H, W_)), torch.tensor(y).view(y.shape[:2] + (H, W_))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))


# ------------------------------------------------------------------------------------------------------------------ the definition

@pytest.mark.parametrize("M", [1, 2, 5, 8])
def test_the_definition_is_the_integral_of_the_squared_cdf_difference(M):
    """crps = A - B / M^2 against integral (F_M(z) - 1[z >= y])^2 dz, the step function integrated exactly in float64: random cells,
    cells with ties among the members and with the truth, and the truth below and above the whole ensemble"""
    rng = np.random.default_rng(M)
    cases = []
    for i in range(200):
        x = rng.standard_normal(M) * rng.uniform(0.1, 3.0) + rng.uniform(-5, 5)
        y = rng.standard_normal() * 2.0
        if i % 4 == 1:
            x = np.round(x)            # ties among the members
            y = x[i % M] if i % 8 == 1 else np.round(y)
        if i % 4 == 2:
            y = x.min() - rng.uniform(0.0, 4.0)  # outside, below (and at the edge when the draw is 0)
        if i % 4 == 3:
            y = x.max() + rng.uniform(0.0, 4.0)
        cases.append((x.astype(np.float32), np.float32(y)))
    cases.append((np.full(M, 2.5, np.float32), np.float32(2.5)))   # everything in one point: 0
    cases.append((np.full(M, 2.5, np.float32), np.float32(-1.0)))  # identical members: |x - y|
    worst = 0.0
    for x, y in cases:
        t = R.terms64(x[:, None], np.array([y]))[:, 0]
        closed = t[0] - t[1] / M ** 2
        want = R.crps_integral(x, y)
        scale = max(abs(want), t[0])
        rel = abs(closed - want) / scale if scale > 0 else abs(closed - want)
        worst = max(worst, rel)
        assert rel <= 1e-12, (x, y, closed, want)
        assert t[2] <= t[0] ** 2 * (1 + 1e-12)  # E <= A^2: what the rule for E leans on
    print(f"M = {M}: A - B / M^2 against the exact integral over {len(cases)} cells: worst relative difference {worst:.3g}")
    assert R.crps_integral(np.full(M, 2.5), -1.0) == pytest.approx(3.5, rel=1e-15)


def test_the_sorted_gap_form_of_b_is_the_pair_sum():
    rng = np.random.default_rng(3)
    for M in (2, 3, 8, 17, 64):
        x = np.round(rng.standard_normal((M, 50)) * 4.0) / 4.0  # with ties
        s = np.sort(x, axis=0)
        k = np.arange(1, M)[:, None]
        gaps = (k * (M - k) * (s[1:] - s[:-1])).sum(axis=0)
        pairs = R.terms64(x.astype(np.float32), np.zeros(50, np.float32))[1]
        assert np.allclose(gaps, pairs, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------------------------ both routes

SHAPES = [(1, 1, 1, 2, 2), (3, 3, 2, 8, 8), (8, 2, 3, 16, 12), (17, 2, 2, 4, 4), (64, 1, 2, 4, 8), (5, 1, 1, 41, 100)]


@pytest.mark.parametrize("M,T,F,H,W_", SHAPES)
def test_every_field_kind_against_float64(route, M, T, F, H, W_):
    """hw = 4, 64, 192, 16, 32 and 4100 (two chunks of the launcher's, the second of four cells); every (K, V) of the kernel"""
    for kind in R.KINDS:
        x, y, cells64, sums64, s_cells, s_sums = R.reference(kind, M, T, F, H * W_)
        S, Tr = _t5(x, y, H, W_)
        sums, cells = C.ensemble_terms(S, Tr, cells=True)
        assert sums.dtype == torch.float64 and sums.shape == (T, F, 4) and cells.dtype == torch.float32 and cells.shape == (4, T, F, H, W_)
        rc, ok_c = R.worst(cells.numpy().reshape(4, T, F, -1), cells64, s_cells, M)
        rs, ok_s = R.worst(sums.numpy(), sums64, s_sums, M)
        print(f"{route} {kind} {(M, T, F, H * W_)}: error over (M + 16) 2^-24 s (limit 1): cells {rc:.3g}, sums {rs:.3g}")
        assert ok_c and ok_s, (kind, rc, rs)
        assert _same_bits(C.ensemble_terms(S, Tr).numpy(), sums.numpy())  # without the cells: the same sums
        if kind == "ties":
            same = (x == x[:1]).all(axis=0)
            assert same.any() and np.all(cells.numpy().reshape(4, T, F, -1)[1][same] == 0)
            if M > 1:
                assert np.all(cells.numpy().reshape(4, T, F, -1)[3][same] == 0)  # identical members: B == 0 and V == 0 exactly


def _straight_port32(x, y):
    """the straight fp32 port the rule must refuse: the mean and the variance on the raw values, summed in member order"""
    M = x.shape[0]
    f32 = np.float32
    total = np.zeros_like(y)
    for m in range(M):
        total = total + x[m]
    mean = total / f32(M)
    ss = np.zeros_like(y)
    for m in range(M):
        d = x[m] - mean
        ss = ss + d * d
    assert mean.dtype == f32 and ss.dtype == f32
    return (mean - y) * (mean - y), ss / f32(M - 1)


@pytest.mark.parametrize("M", [8, 17, 64])
def test_the_straight_fp32_port_fails_the_rule_where_the_kernel_s_arithmetic_passes(M, monkeypatch):
    """pressure-like fields with the ensemble 50 spreads off the truth: the mean of raw values near 101325 is off by several 2^-8, which
    E = (mean - y)^2 and V see in full"""
    T, F, hw = 2, 2, 256
    x, y, cells64, sums64, s_cells, s_sums = R.reference("pressure_biased", M, T, F, hw)
    e32, v32 = _straight_port32(x, y)
    re_, ok_e = R.worst(e32, cells64[2], s_cells[2], M)
    rv, ok_v = R.worst(v32, cells64[3], s_cells[3], M)
    print(f"pressure_biased M = {M}: straight fp32 port, error over the bound (limit 1): E {re_:.3g}, V {rv:.3g}")
    assert not ok_e and not ok_v and re_ > 1.5 and rv > 1.5
    emu_crps_ops.install(monkeypatch, c2w_ops, C)
    _, cells = C.ensemble_terms(*_t5(x, y, 16, 16), cells=True)
    rk, ok = R.worst(cells.numpy().reshape(4, T, F, hw), cells64, s_cells, M)
    print(f"pressure_biased M = {M}: the kernel's arithmetic (emulated), error over the bound: {rk:.3g}")
    assert ok and emu_crps_ops.CALLS == [(M, T, F, hw, True)]


def test_derived_scores_are_the_same_algebra_in_float64(route):
    M, T, F, H, W_ = 8, 3, 2, 8, 8
    x, y, cells64, sums64, s_cells, s_sums = R.reference("temperature", M, T, F, H * W_)
    S, Tr = _t5(x, y, H, W_)
    sums = C.ensemble_terms(S, Tr).numpy()
    want = R.scores64(sums, M, H * W_)
    assert np.allclose(C.crps(S, Tr).numpy(), want["crps"], rtol=1e-14, atol=0) and C.crps(S, Tr).shape == (T, F)
    assert np.allclose(C.crps(S, Tr, fair=True).numpy(), want["crps_fair"], rtol=1e-14, atol=0)
    rmse, spread, ratio = C.spread_skill(S, Tr)
    for got, key in ((rmse, "rmse"), (spread, "spread"), (ratio, "ratio")):
        assert got.shape == (F,) and got.dtype == torch.float64 and np.allclose(got.numpy(), want[key], rtol=1e-14, atol=0)
    truth = R.scores64(sums64, M, H * W_)  # and against the float64 definition: crps to a few (M + 16) 2^-24 of mean A
    assert np.all(np.abs(C.crps(S, Tr).numpy() - truth["crps"]) <= 2 * R.factor(M) * sums64[..., 0] / (H * W_))
    assert np.all(C.crps(S, Tr, fair=True).numpy() <= C.crps(S, Tr).numpy())  # the fair form takes more of B away
    assert C.consistency_factor(M) == np.sqrt((M + 1) / M)


def test_one_member_and_no_members(route):
    x, y = R.fields("wind", 1, 2, 2, 16)
    S, Tr = _t5(x, y, 4, 4)
    sums = C.ensemble_terms(S, Tr)
    assert torch.isnan(sums[..., 3]).all() and not torch.isnan(sums[..., :3]).any() and torch.all(sums[..., 1] == 0)
    assert np.allclose(C.crps(S, Tr).numpy(), np.abs(x[0].astype(np.float64) - y).mean(axis=-1), rtol=1e-6)  # M = 1: the absolute error
    assert torch.isnan(C.crps(S, Tr, fair=True)).all()
    rmse, spread, ratio = C.spread_skill(S, Tr)
    assert not torch.isnan(rmse).any() and torch.isnan(spread).all() and torch.isnan(ratio).all()
    none = C.ensemble_terms(S[:0], Tr)
    assert none.shape == (2, 2, 4) and torch.isnan(none).all() and torch.isnan(C.crps(S[:0], Tr)).all()
    assert C.ensemble_terms(S[:, :0], Tr[:0]).shape == (0, 2, 4)


def test_a_non_finite_value_poisons_its_own_entry_only(route):
    M, T, F, H, W_ = 5, 3, 2, 8, 8
    x, y = R.fields("wind", M, T, F, H * W_)
    S, Tr = _t5(x.copy(), y.copy(), H, W_)
    clean, clean_cells = C.ensemble_terms(S, Tr, cells=True)
    S[2, 1, 0, 3, 3] = float("nan")
    S[0, 2, 1, 0, 0] = float("-inf")
    Tr[0, 1, 7, 7] = float("inf")
    sums, cells = C.ensemble_terms(S, Tr, cells=True)
    bad = torch.zeros(T, F, dtype=torch.bool)
    bad[1, 0] = bad[2, 1] = bad[0, 1] = True
    assert torch.equal(torch.isnan(sums).all(dim=-1), bad) and torch.equal(torch.isnan(sums).any(dim=-1), bad)
    assert torch.equal(sums[~bad], clean[~bad])
    bad_cells = torch.zeros(T, F, H, W_, dtype=torch.bool)
    bad_cells[1, 0, 3, 3] = bad_cells[2, 1, 0, 0] = bad_cells[0, 1, 7, 7] = True
    assert torch.equal(torch.isnan(cells).all(dim=0), bad_cells) and torch.equal(torch.isnan(cells).any(dim=0), bad_cells)
    assert torch.equal(cells[:, ~bad_cells], clean_cells[:, ~bad_cells])
    assert torch.equal(torch.isnan(C.crps(S, Tr)), bad)


def test_any_dtype_any_strides(route):
    base = 280.0 + 10.0 * torch.randn(4, 3, 2, 8, 16, dtype=torch.float64)
    truth_base = 280.0 + 10.0 * torch.randn(3, 2, 8, 16, dtype=torch.float64)
    view, tview = base[..., ::2], truth_base[..., 1::2]  # strided
    for cast in (torch.float64, torch.float16, torch.bfloat16):
        S, Tr = view.to(cast), tview.to(cast)
        x32, y32 = S.float().numpy().reshape(4, 3, 2, 64), Tr.float().numpy().reshape(3, 2, 64)
        cells64 = R.terms64(x32, y32)
        sums, cells = C.ensemble_terms(S, Tr, cells=True)
        assert R.worst(cells.numpy().reshape(4, 3, 2, 64), cells64, R.yardsticks(cells64), 4)[1], cast
        assert R.worst(sums.numpy(), np.moveaxis(cells64.sum(-1), 0, -1), np.moveaxis(R.yardsticks(cells64).sum(-1), 0, -1), 4)[1], cast


# ------------------------------------------------------------------------------------------------------------------ report

def test_report_keys_and_values(route):
    M, T, F, H, W_ = 8, 4, 2, 8, 8
    x, y, cells64, sums64, s_cells, s_sums = R.reference("pressure", M, T, F, H * W_)
    S, Tr = _t5(x, y, H, W_)
    rep = C.crps_report(S, Tr, names=["psl", "psl2"])
    sums = C.ensemble_terms(S, Tr).numpy()
    n = T * H * W_
    tot = sums.sum(axis=0)
    assert rep.names == ["psl", "psl2"] and not hasattr(rep, "all_variables")
    for f, (name, v) in enumerate(rep):
        assert set(v) == {"crps", "crps_fair", "rmse", "spread", "ratio", "crps_by_time"} and rep[name] is v
        assert all(t.dtype == torch.float64 for t in v.values()) and v["crps_by_time"].shape == (T,) and v["crps"].dim() == 0
        assert float(v["crps"]) == pytest.approx((tot[f, 0] - tot[f, 1] / M ** 2) / n, rel=1e-14)
        assert float(v["crps_fair"]) == pytest.approx((tot[f, 0] - tot[f, 1] / (M * (M - 1))) / n, rel=1e-14)
        assert float(v["rmse"]) == pytest.approx(np.sqrt(tot[f, 2] / n), rel=1e-14)
        assert float(v["spread"]) == pytest.approx(np.sqrt(tot[f, 3] / n), rel=1e-14)
        assert float(v["ratio"]) == pytest.approx(np.sqrt((M + 1) / M) * np.sqrt(tot[f, 3] / tot[f, 2]), rel=1e-14)
        assert np.allclose(v["crps_by_time"].numpy(), (sums[:, f, 0] - sums[:, f, 1] / M ** 2) / (H * W_), rtol=1e-14, atol=0)
        assert float(v["crps_by_time"].mean()) == pytest.approx(float(v["crps"]), rel=1e-12)  # equal planes: the mean of the means
        f64 = R.scores64(sums64, M, H * W_)
        assert abs(float(v["rmse"]) - f64["rmse"][f]) <= R.factor(M) * f64["rmse"][f] * 4  # sqrt halves a relative error; A^2 / E is small here
        assert 0.8 < float(v["ratio"]) < 1.25  # the truth is one more draw from each cell's ensemble: consistent by construction
    flat = rep.as_dict()
    assert set(flat) == {f"crps/{n_}/{k}" for n_ in ("psl", "psl2") for k in ("crps", "crps_fair", "rmse", "spread", "ratio")}
    assert all(isinstance(val, float) for val in flat.values())
    assert flat["crps/psl2/spread"] == float(rep["psl2"]["spread"]) and set(rep.as_dict("eval")) >= {"eval/psl/ratio"}
    assert C.crps_report(S, Tr).names == ["var0", "var1"]


def test_argument_checks():
    x, y = torch.zeros(3, 2, 2, 8, 8), torch.zeros(2, 2, 8, 8)
    for fn in (C.ensemble_terms, C.crps, C.spread_skill, C.crps_report):
        with pytest.raises(ValueError, match=r"\(3, 2, 2, 8, 4\)"):
            fn(x[..., :4], y)
        with pytest.raises(ValueError):
            fn(x[0], y)
        with pytest.raises(ValueError):
            fn(x, y[0])
        with pytest.raises(ValueError):
            fn(x.long(), y)
    with pytest.raises(ValueError, match="1 names for 2 variables"):
        C.crps_report(x, y, names=["only_one"])


def test_unsupported_shapes_take_the_general_route(monkeypatch):
    """hw no multiple of 4, M > 64 and M == 0: the launcher is asked, answers no, nothing is launched, the general route answers"""
    emu_crps_ops.install(monkeypatch, c2w_ops, C)
    for M, H, W_ in ((3, 5, 5), (65, 4, 4)):
        x, y = R.fields("wind", M, 2, 2, H * W_)
        cells64 = R.terms64(x, y)
        sums, cells = C.ensemble_terms(*_t5(x, y, H, W_), cells=True)
        assert R.worst(cells.numpy().reshape(cells64.shape), cells64, R.yardsticks(cells64), M)[1]
        assert np.allclose(sums.numpy(), np.moveaxis(cells64.sum(-1), 0, -1), rtol=1e-13, atol=0)
    assert emu_crps_ops.CALLS == []  # crps_supported said no before anything was allocated
    assert not emu_crps_ops.crps_terms(None, None, None, None, None, 65, 2, 2, 16) and not emu_crps_ops.crps_terms(None, None, None, None, None, 3, 2, 2, 25)


# ------------------------------------------------------------------------------------------------------------------ the kernels' maps

@pytest.fixture(scope="module")
def host_crps(tmp_path_factory):
    """a stand-alone program under the address and undefined-behaviour sanitizers; it is run directly, never loaded into Python.
    -ffp-contract=off: the kernel fuses no multiply with an add either (crps_core.h says so to its own compiler)."""
    return host_program.build(tmp_path_factory, "crps", sanitize=True, fp_contract_off=True, timeout=600)


@pytest.mark.parametrize("M,T,F,hw", [(1, 2, 2, 4), (8, 3, 2, 100), (9, 2, 2, 1028), (16, 1, 3, 4100), (17, 2, 1, 520), (32, 1, 2, 4100), (33, 2, 1, 260),
                                      (64, 1, 1, 4100), (64, 2, 2, 8196)])
def test_every_cell_of_every_plane_is_fetched_exactly_once(host_crps, tmp_path, M, T, F, hw):
    """every (K, V) on both sides of its boundary, planes smaller than one round, planes of one chunk + 4 cells and of two chunks + 4
    (three workgroups a plane).  The fields hold their own indices, so what was fetched says where from."""
    subprocess.run([str(host_crps), "visit", str(M), str(T), str(F), str(hw), str(tmp_path / "ox.i32"), str(tmp_path / "oy.i32")], check=True, timeout=600)
    ox, oy = np.fromfile(tmp_path / "ox.i32", dtype=np.int32), np.fromfile(tmp_path / "oy.i32", dtype=np.int32)
    plane = np.arange(T * F).reshape(T, F, 1)
    assert np.array_equal(ox.reshape(M, T, F, hw), np.broadcast_to(plane[None], (M, T, F, hw)))
    assert np.array_equal(oy.reshape(T, F, hw), np.broadcast_to(plane, (T, F, hw)))


@pytest.mark.parametrize("M,T,F,hw", [(1, 2, 1, 8), (3, 2, 2, 64), (8, 1, 2, 4100), (16, 2, 1, 192), (17, 1, 1, 4100), (33, 1, 2, 516), (64, 1, 1, 4100)])
def test_terms_on_the_host_equal_the_emulation_bit_for_bit(host_crps, tmp_path, M, T, F, hw):
    """csrc/crps_core.h compiled for the host against tests/emu_crps_ops.py: the sorting network, the arithmetic, the accumulation
    order, the fold through LDS and over the chunks; every kind, with and without the per-cell output"""
    for kind in R.KINDS:
        x, y = R.fields(kind, M, T, F, hw)
        x.tofile(tmp_path / "x"), y.tofile(tmp_path / "y")
        X, Y = torch.tensor(x), torch.tensor(y)
        sums = torch.full((T, F, 4), -7.25, dtype=torch.float64)
        cells = torch.full((4, T, F, hw), -7.25)
        nbytes = emu_crps_ops.crps_scratch_bytes(T, F, hw)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64) if nbytes else None
        assert emu_crps_ops.crps_terms(X, Y, sums, cells, scratch, M, T, F, hw)
        for with_cells in (1, 0):
            subprocess.run([str(host_crps), "terms", str(M), str(T), str(F), str(hw), str(with_cells)] + [str(tmp_path / n) for n in ("x", "y", "sums", "cells")],
                           check=True, timeout=600)
            assert _same_bits(np.fromfile(tmp_path / "sums", dtype=np.float64).reshape(T, F, 4), sums.numpy()), (kind, with_cells)
            if with_cells:
                assert _same_bits(np.fromfile(tmp_path / "cells", dtype=np.float32).reshape(4, T, F, hw), cells.numpy()), kind


def test_support_predicate_and_chunking_agree():
    for hw, M, want in ((4, 1, True), (16384, 64, True), (66, 8, False), (64, 65, False), (64, 0, False), (0, 8, False)):
        assert emu_crps_ops.crps_supported(hw, M) is want
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "crps_core.h")).read()
    for text in ("THREADS = 256", "MAX_M = 64", "CHUNK = 4096", "hw % 4 == 0 && M >= 1 && M <= MAX_M",
                 "M <= 8 ? 8 : M <= 16 ? 16 : M <= 32 ? 32 : 64", "K <= 16 ? 4 : K == 32 ? 2 : 1"):
        assert text in core, text
    shared = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "ordered_sum.h")).read()
    for text in ("THREADS = 256", "GROUP = 16"):
        assert text in shared, text
    assert [emu_crps_ops.rows_of(M) for M in (1, 8, 9, 16, 17, 32, 33, 64)] == [8, 8, 16, 16, 32, 32, 64, 64]
    assert [emu_crps_ops.chunks(hw) for hw in (4, 4096, 4100, 16384)] == [1, 1, 2, 4]  # a function of hw alone
    assert emu_crps_ops.crps_scratch_bytes(1457, 4, 16384) == 1457 * 4 * 4 * 4 * 8 and emu_crps_ops.crps_scratch_bytes(1457, 4, 4096) == 0


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_crps_supported": "int", "c2w_crps_scratch_bytes": "long long", "c2w_crps_terms": "int"}
    c_abi.assert_declared(names, "crps.hip", c2w_ops, ("crps_supported", "crps_scratch_bytes", "crps_terms"))
