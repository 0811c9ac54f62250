"""CPU checks of the temporal increment scores (climate2weather_amd.temporal): the known answers -- a ramp, the expansion of the
square, time reversal, a constant per cell, members equal to the truth, a spike at every sixth hour -- all exact; both routes of every
public function -- the general float64 one and the launcher's, with tests/emu_temporal_ops.py standing in for the HIP kernel -- against
the float64 table by the rules of tests/fp64_temporal_ref.py; the edge cases; the kernel's own index maps and arithmetic compiled for
the host (csrc/temporal_core.h), once plain and once under the address and undefined-behaviour sanitizers; and the C declarations
against the ctypes prototypes."""
import os
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_temporal_ops
import fp64_temporal_ref as R
import host_program
from climate2weather_amd import temporal as TP
from climate2weather_amd import temporal_ops
from climate2weather_amd.ensemble_host import VariableReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of temporal.increment_terms on CPU tensors"""
    if request.param == "launcher":
        emu_temporal_ops.install(monkeypatch, temporal_ops, TP)
    return request.param


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))


def _t5(x, y, H, W_):
    """(M, T, F, hw), (T, F, hw) arrays -> the (M, T, F, H, W), (T, F, H, W) tensors of the public interface"""
    return torch.tensor(x).view(x.shape[:3] + (H, W_)), None if y is None else torch.tensor(y).view(y.shape[:2] + (H, W_))


def _integers(M, T, F, H, W_, seed=0, top=9):
    """small-integer fields: every difference, square and sum below is exact in fp32 and in float64"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-top, top + 1, (M, T, F, H, W_), generator=g).float(), torch.randint(-top, top + 1, (T, F, H, W_), generator=g).float())


# ------------------------------------------------------------------------------------------------------------------ known answers

@pytest.mark.parametrize("b", [0.25, -2.0])
def test_a_ramp_has_the_structure_functions_b_tau_and_b2_tau2(route, b):
    M, T, F, H, W_, L = 2, 9, 2, 4, 6, 8
    a = torch.arange(H * W_, dtype=torch.float32).view(1, 1, 1, H, W_) / 8.0
    t = torch.arange(T, dtype=torch.float32).view(1, T, 1, 1, 1)
    x = (a + b * t + torch.arange(F).view(1, 1, F, 1, 1)).expand(M, T, F, H, W_).contiguous()
    s1, s2 = TP.structure_functions(x, None, L)
    tau = torch.arange(1, L + 1, dtype=torch.float64)
    assert s1.shape == s2.shape == (M, F, L) and s1.dtype == torch.float64
    assert torch.equal(s1, (abs(b) * tau).expand(M, F, L)) and torch.equal(s2, (b * b * tau * tau).expand(M, F, L))
    late = TP.structure_functions(x[:, :3], None, L)  # T = 3: the lags from 3 on have no pair
    assert torch.isnan(late[0][..., 2:]).all() and torch.isnan(late[1][..., 2:]).all() and torch.equal(late[0][..., :2], s1[..., :2])


def test_the_square_of_an_increment_expands_on_small_integers(route):
    M, T, F, H, W_, L = 3, 7, 2, 4, 5, 4
    x, y = _integers(M, T, F, H, W_, seed=1)
    S = TP.increment_terms(x, y, L)
    rows = torch.cat([y[None], x]).double().flatten(-2)
    for tau in range(1, L + 1):
        a, b = rows[:, :-tau], rows[:, tau:]
        want = (b * b).sum(-1) + (a * a).sum(-1) - 2.0 * (a * b).sum(-1)
        assert torch.equal(S[:, :T - tau, :, tau - 1, 1], want)
        assert torch.equal(S[:, :T - tau, :, tau - 1, 0], (b - a).abs().sum(-1))
        assert torch.equal(S[:, :T - tau, :, tau - 1, 2], ((b - a) - (b - a)[:1]).pow(2).sum(-1))
        assert torch.all(S[:, T - tau:, :, tau - 1] == 0)


def test_time_reversal_maps_the_anchors_and_keeps_the_pooled_functions(route):
    M, T, F, H, W_, L = 2, 8, 2, 4, 4, 5
    x, y = _integers(M, T, F, H, W_, seed=2)
    S, Sr = TP.increment_terms(x, y, L), TP.increment_terms(x.flip(1), y.flip(0), L)
    for tau in range(1, L + 1):
        for t in range(T - tau):
            assert torch.equal(Sr[:, T - 1 - t - tau, :, tau - 1], S[:, t, :, tau - 1]), (t, tau)
    for a, b in zip(TP.structure_functions(x, y, L), TP.structure_functions(x.flip(1), y.flip(0), L)):
        assert torch.equal(a, b)
    assert torch.equal(TP.tendency_rmse(x, y, L), TP.tendency_rmse(x.flip(1), y.flip(0), L))


def test_a_constant_per_cell_leaves_the_table_unchanged(route):
    M, T, F, H, W_, L = 2, 6, 2, 4, 4, 3
    x, y = _integers(M, T, F, H, W_, seed=3)
    g = torch.Generator().manual_seed(4)
    cx = torch.randint(-50, 51, (M, 1, F, H, W_), generator=g).float() * 64.0  # per cell, the same at every hour; the sums stay exact in fp32
    cy = torch.randint(-50, 51, (1, F, H, W_), generator=g).float() * 64.0
    assert torch.equal(TP.increment_terms(x + cx, y + cy, L), TP.increment_terms(x, y, L))


def test_members_equal_to_the_truth_have_no_tendency_error_and_ratio_one(route):
    M, T, F, H, W_, L = 3, 7, 2, 4, 8, 4
    y = torch.tensor(R.fields("temperature", 1, T, F, H * W_)[1]).view(T, F, H, W_)
    x = y[None].expand(M, -1, -1, -1, -1).contiguous()
    S = TP.increment_terms(x, y, L)
    assert torch.all(S[..., 2] == 0) and not torch.signbit(S[..., 2]).any()
    assert torch.all(TP.tendency_rmse(x, y, L) == 0)
    for order in (1, 2):
        ratio = TP.variability_ratio(x, y, L, order=order)
        assert ratio.shape == (M, F, L) and torch.all(ratio == 1.0)
    smooth = y[None] * 0.5  # half the increments: both ratios are exactly 1 / 2
    assert torch.all(TP.variability_ratio(smooth, y, L, order=2) == 0.5) and torch.all(TP.variability_ratio(smooth, y, L, order=1) == 0.5)


def test_a_spike_at_every_sixth_hour_shows_at_lag_1_before_and_at_the_observation(route):
    M, T, F, H, W_, L = 2, 25, 1, 4, 4, 3
    x = torch.zeros(M, T, F, H, W_)
    x[:, ::6] = 2.0
    y = torch.zeros(T, F, H, W_)
    means, counts = TP.by_phase(TP.increment_terms(x, y, L), period=6)
    assert means.shape == (M + 1, 6, F, L, 3) and counts.shape == (6, L)
    assert counts[:, 0].tolist() == [4.0, 4.0, 4.0, 4.0, 4.0, 4.0] and counts[:, 2].tolist() == [4.0, 4.0, 4.0, 4.0, 3.0, 3.0]
    lag1 = means[1:, :, 0, 0]  # (M, phi, column)
    hw = H * W_
    for phi in range(6):
        want = torch.tensor([2.0 * hw, 4.0 * hw, 4.0 * hw], dtype=torch.float64) if phi in (5, 0) else torch.zeros(3, dtype=torch.float64)
        assert torch.equal(lag1[0, phi], want) and torch.equal(lag1[1, phi], want), phi
    assert torch.all(means[0] == 0)  # the truth does not move
    late = torch.zeros(M, T, F, H, W_)
    late[:, 2::6] = 2.0  # the observations at hours 2, 8, ..: offset 2
    shifted, _ = TP.by_phase(TP.increment_terms(late, y, L), period=6, offset=2)
    assert torch.equal(shifted[1:, 1:5, 0, 0], torch.zeros_like(shifted[1:, 1:5, 0, 0])) and torch.all(shifted[1:, 5, 0, 0, 0] == 2.0 * hw)
    none, n0 = TP.by_phase(TP.increment_terms(x[:, :3], y[:3], L), period=6)
    assert n0[3:].sum() == 0 and torch.isnan(none[:, 3:]).all() and not torch.isnan(none[:, :2, :, 0]).any()


# ------------------------------------------------------------------------------------------------------------------ both routes

SHAPES = [(2, 5, 2, 4, 4, 3), (1, 9, 1, 41, 100, 8), (3, 4, 2, 64, 64, 9), (2, 3, 1, 8, 8, 24)]


@pytest.mark.parametrize("M,T,F,H,W_,L", SHAPES)
def test_every_field_kind_against_float64(route, M, T, F, H, W_, L):
    """hw = 16, 4100 (two chunks, the last of four cells), 4096 and 64; L below, at and beyond a fold pass and beyond T - 1"""
    for kind in R.KINDS:
        x, y, S, Y = R.reference(kind, M, T, F, H * W_, L)
        got = TP.increment_terms(*_t5(x, y, H, W_), max_lag=L)
        assert got.dtype == torch.float64 and got.shape == (M + 1, T, F, L, 3)
        r, ok = R.worst_table(got.numpy(), S, Y, H * W_)
        print(f"{route} {kind} {(M, T, F, H * W_, L)}: error over the rules (limit 1): A1 {r[0]:.3g}, A2 {r[1]:.3g}, E2 {r[2]:.3g}")
        assert ok, (kind, r)
        if kind == "nonfinite":
            assert np.isnan(S).any() and not np.isnan(S).all()
        if kind == "constant":
            assert np.all(got.numpy() == 0)


def test_without_a_truth_the_third_column_is_zero(route):
    for kind in ("pressure", "nonfinite"):
        x, _, S, Y = R.reference(kind, 2, 5, 2, 16, 4, with_truth=False)
        got = TP.increment_terms(torch.tensor(x).view(2, 5, 2, 4, 4), None, 4)
        assert got.shape == (2, 5, 2, 4, 3) and torch.all(got[..., 2] == 0) and not torch.signbit(got[..., 2]).any()
        assert R.worst_table(got.numpy(), S, Y, 16)[1]
    lead = torch.tensor(R.fields("wind", 6, 4, 1, 16)[0]).view(2, 3, 4, 1, 4, 4)  # any leading shape: one data set per index
    assert torch.equal(TP.increment_terms(lead, None, 2), TP.increment_terms(lead.view(6, 4, 1, 4, 4), None, 2))


@pytest.mark.parametrize("T", [1, 2])
def test_short_series_and_lags_beyond_the_series(route, T):
    M, F, H, W_, L = 1, 2, 4, 4, 5
    x, y = _integers(M, T, F, H, W_, seed=5)
    S = TP.increment_terms(x, y, L)
    assert S.shape == (M + 1, T, F, L, 3)
    if T == 1:
        assert torch.all(S == 0) and not torch.signbit(S).any()
    else:
        assert torch.equal(S[1, 0, :, 0, 1], (x[0, 1] - x[0, 0]).double().pow(2).sum((-2, -1))) and torch.all(S[:, 1] == 0) and torch.all(S[:, 0, :, 1:] == 0)
    s1, s2 = TP.structure_functions(x, y, L)
    assert torch.isnan(s1[..., T - 1:]).all() and not torch.isnan(s1[..., :T - 1]).any()
    assert TP.tendency_rmse(x, y, L).shape == (M, F, L)
    assert TP.increment_terms(x[:0], y, L).shape == (1, T, F, L, 3) and TP.increment_terms(x[:0], None, L).shape == (0, T, F, L, 3)


def test_a_non_finite_value_poisons_its_own_entries_only(route):
    M, T, F, H, W_, L = 3, 8, 2, 4, 4, 3
    x, y = _integers(M, T, F, H, W_, seed=6)
    clean = TP.increment_terms(x, y, L)
    x, y = x.clone(), y.clone()
    x[1, 4, 0, 2, 2] = float("nan")   # row 2, in the middle: three lags forward, three backward
    x[2, 7, 1, 0, 0] = float("-inf")  # row 3, the last hour: backward only
    y[1, 1, 3, 3] = float("inf")      # the truth: one lag backward, three forward, column 2 of every row
    S = TP.increment_terms(x, y, L)

    def poisoned(planes, rows, columns):
        bad = torch.zeros(rows, T, F, L, 3, dtype=torch.bool)
        for d, t, f in planes:
            for tau in range(1, L + 1):
                for anchor in (t, t - tau):
                    if 0 <= anchor and anchor + tau < T:
                        bad[d, anchor, f, tau - 1, :columns] = True
                        if d == 0 and columns == 3:
                            bad[:, anchor, f, tau - 1, 2] = True
        return bad

    bad = poisoned(((2, 4, 0), (3, 7, 1), (0, 1, 1)), M + 1, 3)
    assert torch.equal(torch.isnan(S), bad) and torch.equal(S[~bad], clean[~bad])
    assert int(bad[1].sum()) == 4 and int(bad[3, :, 1].sum()) == 9 + 4  # an untouched member: only the third column of the truth's four entries
    no_truth = TP.increment_terms(x, None, L)  # the rows are the members alone; the third column stays +0.0
    assert torch.equal(torch.isnan(no_truth), poisoned(((1, 4, 0), (2, 7, 1)), M, 2)) and torch.all(no_truth[..., 2] == 0)


def test_any_dtype_any_strides(route):
    base = 280.0 + 10.0 * torch.randn(3, 6, 2, 8, 32, dtype=torch.float64)
    truth_base = 280.0 + 10.0 * torch.randn(6, 2, 8, 32, dtype=torch.float64)
    view, tview = base[..., ::2], truth_base[..., 1::2]  # strided
    for cast in (torch.float64, torch.float16, torch.bfloat16):
        S_, Tr = view.to(cast), tview.to(cast)
        want, Y = R.table64(S_.float().numpy().reshape(3, 6, 2, -1), Tr.float().numpy().reshape(6, 2, -1), 4)
        assert R.worst_table(TP.increment_terms(S_, Tr, 4).numpy(), want, Y, 128)[1], cast


# ------------------------------------------------------------------------------------------------------------------ report

def test_report_keys_and_values(route):
    M, T, F, H, W_, L = 3, 13, 2, 4, 8, 4
    x, y = R.fields("temperature", M, T, F, H * W_)
    S_, Tr = _t5(x, y, H, W_)
    rep = TP.temporal_report(S_, Tr, names=["tas", "psl"], max_lag=L, period=6)
    assert isinstance(rep, VariableReport) and rep.names == ["tas", "psl"]
    s1, s2 = TP.structure_functions(S_, Tr, L)
    r1, r2, rmse = TP.variability_ratio(S_, Tr, L, order=1), TP.variability_ratio(S_, Tr, L), TP.tendency_rmse(S_, Tr, L)
    means, counts = TP.by_phase(TP.increment_terms(S_, Tr, L), 6)
    for f, (name, v) in enumerate(rep):
        assert set(v) == {"structure_1_truth", "structure_2_truth", "structure_1", "structure_2", "ratio_1", "ratio_2", "tendency_rmse", "phase_mean", "phase_count"}
        assert rep[name] is v and all(t.dtype == torch.float64 for t in v.values())
        assert torch.equal(v["structure_1_truth"], s1[0, f]) and torch.equal(v["structure_2"], s2[1:, f])
        assert torch.equal(v["ratio_1"], r1[:, f]) and torch.equal(v["ratio_2"], r2[:, f]) and torch.equal(v["tendency_rmse"], rmse[:, f])
        assert torch.equal(v["phase_mean"], means[:, :, f] / (H * W_)) and torch.equal(v["phase_count"], counts)
    flat = rep.as_dict()
    assert set(flat) == {f"temporal/{n}/{k}_lag1{s}" for n in ("tas", "psl") for k in ("ratio_1", "ratio_2", "tendency_rmse") for s in ("", "_std")}
    assert flat["temporal/psl/ratio_2_lag1"] == pytest.approx(float(r2[:, 1, 0].mean()), rel=1e-14)
    assert flat["temporal/tas/tendency_rmse_lag1_std"] == pytest.approx(float(rmse[:, 0, 0].std(unbiased=False)), rel=1e-12)
    plain = TP.temporal_report(S_, Tr)
    assert plain.names == ["var0", "var1"] and "phase_mean" not in plain["var0"] and plain["var0"]["ratio_2"].shape == (M, 6)
    assert set(rep.as_dict("eval")) >= {"eval/tas/ratio_1_lag1"}


def test_argument_checks():
    x, y = torch.zeros(3, 4, 2, 8, 8), torch.zeros(4, 2, 8, 8)
    for fn in (TP.increment_terms, TP.structure_functions, TP.variability_ratio, TP.tendency_rmse, TP.temporal_report):
        with pytest.raises(ValueError):
            fn(x[..., :4], y)
        with pytest.raises(ValueError):
            fn(x, y[0])
        with pytest.raises(ValueError):
            fn(x.long(), y)
        with pytest.raises(ValueError, match="max_lag"):
            fn(x, y, max_lag=0)
    with pytest.raises(ValueError):
        TP.increment_terms(x[0, 0, 0])
    with pytest.raises(ValueError):
        TP.temporal_report(x[:0], y)
    with pytest.raises(ValueError, match="order"):
        TP.variability_ratio(x, y, order=3)
    with pytest.raises(ValueError, match="period"):
        TP.by_phase(TP.increment_terms(x, y), 0)
    with pytest.raises(ValueError, match="terms"):
        TP.by_phase(torch.zeros(3, 4, 2, 6), 2)
    with pytest.raises(ValueError, match="1 names for 2 variables"):
        TP.temporal_report(x, y, names=["only_one"])


def test_unsupported_shapes_take_the_general_route(monkeypatch):
    """hw no multiple of 4 and L = 25: the launcher is asked, answers no, nothing is launched, the general route answers with the same
    numbers as it gives on its own"""
    emu_temporal_ops.install(monkeypatch, temporal_ops, TP)
    for H, W_, L in ((2, 3, 4), (4, 4, 25)):
        x, y = R.fields("wind", 2, 30, 2, H * W_)
        S, _ = R.table64(x, y, L)
        got = TP.increment_terms(*_t5(x, y, H, W_), max_lag=L)
        assert np.allclose(got.numpy(), S, rtol=1e-13, atol=0)
    assert emu_temporal_ops.CALLS == []  # tincr_supported said no before anything was allocated
    assert not emu_temporal_ops.tincr_terms(None, None, None, None, 2, 3, 2, 6, 4) and not emu_temporal_ops.tincr_terms(None, None, None, None, 2, 3, 2, 16, 25)
    x, y = R.fields("wind", 2, 5, 1, 16)
    TP.increment_terms(*_t5(x, y, 4, 4), max_lag=24)
    assert emu_temporal_ops.CALLS[-1] == (2, True, 5, 1, 16, 24)


def test_the_general_route_is_the_same_in_every_chunking(monkeypatch):
    """a chunk of one anchor, of three and of the whole series: the same bits"""
    from climate2weather_amd import ensemble_host
    x, y = R.fields("nonfinite", 2, 9, 2, 16)
    whole = TP.increment_terms(*_t5(x, y, 4, 4), max_lag=4)
    for elems in (1, 3 * 3 * 2 * 16):
        monkeypatch.setattr(TP, "chunk_step", lambda per_item, n=elems: max(1, n // max(1, per_item)))
        assert _same_bits(TP.increment_terms(*_t5(x, y, 4, 4), max_lag=4).numpy(), whole.numpy()), elems
    assert ensemble_host.chunk_step(1) == ensemble_host.CHUNK_ELEMS


# ------------------------------------------------------------------------------------------------------------------ the kernel's maps

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_temporal(request, tmp_path_factory):
    """a stand-alone program, once plain and once under the address and undefined-behaviour sanitizers; it is run directly, never loaded
    into Python.  -ffp-contract=off: the kernel fuses no multiply with an add either (temporal_core.h says so to its own compiler)."""
    return host_program.build(tmp_path_factory, "temporal", sanitize=request.param == "sanitized", fp_contract_off=True, timeout=600)


@pytest.mark.parametrize("n_rep,with_y,T,F,hw,L", [(1, 0, 1, 1, 4, 1), (2, 1, 5, 2, 64, 3), (1, 1, 7, 1, 4100, 9), (2, 0, 3, 2, 4096, 24), (1, 1, 30, 1, 8, 24)])
def test_every_cell_and_lag_of_every_anchor_is_visited_exactly_once(host_temporal, n_rep, with_y, T, F, hw, L):
    """a plane smaller than a round, of one chunk and of a chunk + 4 cells; L below a pass, across passes and beyond T - 1; and no lag
    without a pair is taken up"""
    rc = subprocess.run([str(host_temporal), "visit"] + [str(a) for a in (n_rep, with_y, T, F, hw, L)], timeout=600).returncode
    assert rc == 0, f"check {rc} of host_temporal_main.cpp failed"


@pytest.mark.parametrize("hw", [4, 4096, 4100])
def test_the_host_program_equals_the_emulation_bit_for_bit(host_temporal, tmp_path, hw):
    """csrc/temporal_core.h compiled for the host against tests/emu_temporal_ops.py: the rounds, the passes, the arithmetic, the fold
    through LDS and over the chunks; every kind, with and without a truth"""
    M, T, F, L = 2, 7, 2, 9
    for kind in R.KINDS:
        for with_y in (True, False):
            x, y = R.fields(kind, M, T, F, hw)
            x.tofile(tmp_path / "x"), y.tofile(tmp_path / "y")
            D = M + with_y
            S = torch.full((D, T, F, L, 3), -7.25, dtype=torch.float64)
            nbytes = emu_temporal_ops.tincr_scratch_bytes(D, T, F, hw, L)
            scratch = torch.empty(nbytes // 8, dtype=torch.float64) if nbytes else None
            assert emu_temporal_ops.tincr_terms(torch.tensor(x), torch.tensor(y) if with_y else None, S, scratch, M, T, F, hw, L)
            subprocess.run([str(host_temporal), "terms"] + [str(a) for a in (M, int(with_y), T, F, hw, L)] + [str(tmp_path / n) for n in ("x", "y", "S")],
                           check=True, timeout=600)
            assert _same_bits(np.fromfile(tmp_path / "S", dtype=np.float64).reshape(S.shape), S.numpy()), (kind, with_y)


def test_support_predicates_and_maps_agree():
    for hw, L, want in ((4, 1, True), (16384, 24, True), (6, 6, False), (64, 25, False), (64, 0, False), (0, 6, False)):
        assert emu_temporal_ops.tincr_supported(hw, L) is want
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "temporal_core.h")).read()
    for text in ("THREADS = 256", "MAX_L = 24", "CHUNK = 4096", "BATCH = 4", "hw >= 4 && hw % 4 == 0 && L >= 1 && L <= MAX_L"):
        assert text in core, text
    assert [emu_temporal_ops.passes(L) for L in (1, 4, 5, 8, 9, 24)] == [1, 1, 2, 2, 3, 6]
    assert [emu_temporal_ops.chunks(hw) for hw in (4, 4096, 4100, 16384)] == [1, 1, 2, 4]
    assert [emu_temporal_ops.lags_of(7, t, 4) for t in range(7)] == [4, 4, 4, 3, 2, 1, 0]
    assert emu_temporal_ops.tincr_scratch_bytes(9, 7, 2, 16384, 6) == 9 * 7 * 2 * 4 * 18 * 8 and emu_temporal_ops.tincr_scratch_bytes(9, 7, 2, 4096, 6) == 0
    assert R.CHAIN == 0 and "no fp32 chain is kept" in core  # the chain length is a constant of the kernel and enters the bound


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_tincr_supported": "int", "c2w_tincr_scratch_bytes": "long long", "c2w_tincr_terms": "int"}
    c_abi.assert_declared(names, "temporal.hip", temporal_ops, ("tincr_supported", "tincr_scratch_bytes", "tincr_terms"))
