"""Dependence of an ensemble without a GPU (climate2weather_amd/dependence.py, csrc/comoments_maps.h): the co-moment tables of both
routes -- the hour-by-hour torch definition and the emulation of the launcher standing in for the library -- against the NumPy
reference, bit for bit, for every field kind, every F and every cut of the time axis; the sums against rational arithmetic within the
bound comoments_maps.h derives, and the unpivoted one-pass form's miss of it; ``merge`` within its bound; known answers; what the
module and the launcher refuse; and the header compiled for the host as a program of its own, plain and under the sanitizers."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import c_abi
import emu_comoment_ops
import fp64_comoments_ref as R
import host_program
from climate2weather_amd import _lib, build, dependence_ops
from climate2weather_amd import dependence as DP
from climate2weather_amd.ensemble_host import VariableReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of dependence.py on CPU tensors"""
    if request.param == "launcher":
        emu_comoment_ops.install(monkeypatch, dependence_ops, DP)
    return request.param


def _fields(kind, M, T, F, H, W, seed=0):
    x, y = R.field(kind, (M, T, F, H * W), seed), R.field(kind, (T, F, H * W), seed + 1)
    return x, y, torch.from_numpy(x).view(M, T, F, H, W), torch.from_numpy(y).view(T, F, H, W)


def _same(st, t):
    return R.same_bits(st, t.n.numpy(), t.pivot.numpy(), None if t.truth_pivot is None else t.truth_pivot.numpy(), t.sums.numpy(), t.invalid.numpy())


def _state(t):
    """tables as the reference's state dict, cells flattened"""
    D, F = t.pivot.shape[:2]
    return dict(n=t.n.cpu().numpy().reshape(D, -1), pivot=t.pivot.cpu().numpy().reshape(D, F, -1),
                truth_pivot=None if t.truth_pivot is None else t.truth_pivot.cpu().numpy().reshape(D, F, -1),
                sums=t.sums.cpu().numpy().reshape(D, t.sums.shape[1], -1), invalid=t.invalid.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ the tables

@pytest.mark.parametrize("kind", R.KINDS)
def test_the_tables_equal_the_reference_bit_for_bit(route, kind):
    """general route = reference = emulation, as bits: every F the kernel takes, with and without a truth"""
    M, T, H, W = 2, 6, 2, 4
    for F in range(1, 9):
        x, y, xt, yt = _fields(kind, M, T, F, H, W, seed=F)
        for with_truth in (True, False):
            t = DP.comoments(xt, yt if with_truth else None)
            NS = 4 * F + F * (F + 1) // 2 if with_truth else F + F * (F + 1) // 2
            assert t.with_truth == with_truth and tuple(t.sums.shape) == (M + with_truth, NS, H, W) and t.sums.dtype == torch.float64
            assert tuple(t.n.shape) == (M + with_truth, H, W) and t.n.dtype == torch.int32 and tuple(t.pivot.shape) == (M + with_truth, F, H, W)
            assert _same(R.comoments(x, y if with_truth else None), t), (kind, F, with_truth)
    if route == "launcher":
        assert len(emu_comoment_ops.CALLS) == 16 and emu_comoment_ops.CALLS[0] == (M, T, 1, H * W, True)


@pytest.mark.parametrize("kind", ["nan_hours", "late_start", "truth_nan"])
def test_every_cut_of_the_time_axis_gives_the_same_bits(route, kind):
    """T = 7: all 64 ways to cut it into calls, an empty update in front; late_start: the first valid hour lies in a later update"""
    M, T, F, H, W = 1, 7, 2, 1, 4
    x, y, xt, yt = _fields(kind, M, T, F, H, W, seed=3)
    want = R.comoments(x, y)
    for cuts in range(1 << (T - 1)):
        acc = DP.DependenceAccumulator(M, F, H, W).update(xt[:, :0], yt[:0])
        a = 0
        for t in range(1, T + 1):
            if t == T or (cuts >> (t - 1)) & 1:
                acc.update(xt[:, a:t], yt[a:t])
                a = t
        assert _same(want, acc.tables()), cuts
        assert acc.n_times == T


def test_row_zero_carries_the_truth_against_itself(route):
    x, y, xt, yt = _fields("nan_hours", 2, 9, 3, 1, 4, seed=5)
    t = DP.comoments(xt, yt)
    b = DP._blocks(3)
    diag = [k for k, p in enumerate(DP.pair_list(3)) if p[0] == p[1]]
    C, QT, X = t.sums[0, b["C"][0]:b["C"][1]][diag], t.sums[0, b["QT"][0]:b["QT"][1]], t.sums[0, b["X"][0]:b["X"][1]]
    assert torch.equal(C, QT) and torch.equal(C, X) and torch.equal(t.pivot[0], t.truth_pivot[0])
    assert torch.equal(t.sums[0, b["S"][0]:b["S"][1]], t.sums[0, b["ST"][0]:b["ST"][1]])


def test_an_update_longer_than_one_launch_takes_is_walked_in_parts(route, monkeypatch):
    monkeypatch.setattr(DP, "MAX_CALL", 2)
    x, y, xt, yt = _fields("nan_hours", 2, 7, 2, 1, 4, seed=8)
    assert _same(R.comoments(x, y), DP.comoments(xt, yt))
    if route == "launcher":
        assert [c[1] for c in emu_comoment_ops.CALLS] == [2, 2, 2, 1]


def test_tables_works_on_a_copy(route):
    x, y, xt, yt = _fields("inf", 2, 7, 2, 2, 4)
    acc = DP.DependenceAccumulator(2, 2, 2, 4).update(xt[:, :4], yt[:4])
    t = acc.tables()
    t.sums.fill_(1.0), t.n.fill_(7), t.pivot.fill_(3.0), t.invalid.fill_(-1)
    assert _same(R.comoments(x, y), acc.update(xt[:, 4:], yt[4:]).tables())


def test_strided_and_half_precision_inputs(route):
    x, y, xt, yt = _fields("smooth", 2, 6, 2, 2, 4)
    big = torch.zeros((2, 6, 2, 2, 8))
    big[..., ::2] = xt
    a, b = DP.comoments(big[..., ::2], yt), DP.comoments(xt, yt)
    assert torch.equal(a.sums, b.sums) and torch.equal(a.pivot, b.pivot)
    h = DP.comoments(xt.half(), yt.double())
    assert torch.equal(h.sums, DP.comoments(xt.half().float(), yt).sums)


def test_an_unsupported_shape_takes_the_general_route(monkeypatch):
    emu_comoment_ops.install(monkeypatch, dependence_ops, DP)
    assert not dependence_ops.supported(6, 2) and not dependence_ops.supported(8, 9) and dependence_ops.supported(8, 8)
    for F, H, W in ((2, 2, 3), (9, 2, 4)):   # hw = 6; F = 9
        x, y, xt, yt = _fields("nan_hours", 1, 6, F, H, W)
        assert _same(R.comoments(x, y), DP.comoments(xt, yt))
    assert emu_comoment_ops.CALLS == []   # the launcher was asked "supported" only


def test_the_emulation_restates_the_constants_of_the_kernel():
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "comoments_maps.h")).read()
    for text in ("THREADS = 256", "UNROLL = 4", "MAX_F = 8, MAX_T = 1 << 20", "return F <= 1 ? 4 : F <= 2 ? 2 : 1;", "return THREADS * cells_per_thread(F);",
                 "return F + pairs(F) + (truth ? 3 * F : 0);", "hw >= 4 && hw % 4 == 0 && F >= 1 && F <= MAX_F", "& 0x7F800000u) != 0x7F800000u",
                 "return n + (product ? 2 : 1);", "return n_s + (product ? 4 : 3);", "return n_o + (product ? 11 : 6);"):
        assert text in core, text
    e = emu_comoment_ops
    assert (e.THREADS, e.UNROLL, e.MAX_F, e.MAX_T) == (256, 4, 8, 1 << 20) and DP.MAX_CALL == e.MAX_T and DP.MAX_F == e.MAX_F
    assert [e.cells_per_thread(F) for F in range(1, 9)] == [4, 2, 1, 1, 1, 1, 1, 1]
    assert all(e.entries(F, tr) == DP.entries(F, tr) == R.entries(F, tr) for F in range(1, 10) for tr in (True, False))
    assert '#include "core_side.h"' in core and not any(f"#define C2W_{side}" in core for side in ("HD", "BOTH", "CORE_HOST"))
    assert core.index('#include "core_side.h"') < core.index('#include "events_core.h"')


# ------------------------------------------------------------------------------------------------------------------ the bound

@pytest.mark.parametrize("T", [1, 2, 5, 50, 400])
def test_the_sums_lie_within_the_derived_bound(route, T):
    worst = 0.0
    for kind in ("pressure", "smooth", "denormal", "pressure_tight", "huge", "nan_hours"):
        M, F, H, W = (1, 2, 1, 4) if T > 50 else (2, 3, 1, 4)
        x, y, xt, yt = _fields(kind, M, T, F, H, W, seed=T)
        worst = max(worst, R.check_bound(x, y, _state(DP.comoments(xt, yt)), range(H * W)))
        worst = max(worst, R.check_bound(x, None, _state(DP.comoments(xt)), range(H * W)))
    print(f"T = {T} ({route}): worst fraction of the bound {worst:.4f}")


def test_the_unpivoted_one_pass_form_misses_the_bound_at_tight_pressure():
    """101325 +- 0.5 Pa over 400 hours: the central co-moment C - S S / n from the pivoted tables lies within the bound its sums'
    bounds give (fp64_comoments_ref.central_bound); sum xy - sum x sum y / n in float64, formed in the same order, misses it.  At 50
    hours and fewer both forms are exact -- the product of two fp32 values fits a double --, hence the long series."""
    T, F, hw = 400, 2, 4
    x, y, xt, yt = _fields("pressure_tight", 1, T, F, 1, hw, seed=1)
    st = _state(DP.comoments(xt))
    ratios = []
    for c in range(hw):
        hours = R._series(x, None, 0, c)
        P = hours[0][0]
        s, a, _ = R.exact_sums(hours, P, None)            # S0 S1 C00 C01 C11
        n = len(hours)
        exact = s[3] - s[0] * s[1] / n                    # a central sum does not depend on the pivot
        limit = R.central_bound(n, s[0], s[1], s[3], a[0], a[1], a[3])
        S0, S1, C01 = (float(st["sums"][0, k, c]) for k in (0, 1, 3))
        pivoted = C01 - S0 * S1 / n
        u, v = x[0, :, 0, c].astype(np.float64), x[0, :, 1, c].astype(np.float64)
        sx = sy = sxy = 0.0
        for p, q in zip(u, v):
            sx, sy, sxy = sx + p, sy + q, sxy + p * q
        unpivoted = sxy - sx * sy / n
        assert abs(Fraction(pivoted) - exact) <= limit, (c, float(abs(Fraction(pivoted) - exact)), float(limit))
        assert abs(Fraction(unpivoted) - exact) > limit, c
        ratios.append(float(abs(Fraction(unpivoted) - exact) / limit))
    print(f"unpivoted error over the pivoted form's bound: {min(ratios):.3g} .. {max(ratios):.3g}")
    assert min(ratios) > 1e4   # "about 1e8" in the header; four digits of room on this field


# ------------------------------------------------------------------------------------------------------------------ merge

@pytest.mark.parametrize("kind", ["pressure", "smooth", "nan_hours", "late_start", "pressure_tight", "truth_nan"])
def test_merge_lies_within_its_bound(route, kind):
    M, T, F, H, W, cut = 2, 12, 2, 1, 4, 5
    x, y, xt, yt = _fields(kind, M, T, F, H, W, seed=4)
    if kind == "late_start":
        x[:, :cut, :, 2] = np.nan   # a series the first accumulator has no valid hour of
    for with_truth in (True, False):
        yy, yyt = (y, yt) if with_truth else (None, None)
        a = DP.DependenceAccumulator(M, F, H, W, with_truth=with_truth).update(xt[:, :cut], None if yyt is None else yyt[:cut])
        b = DP.DependenceAccumulator(M, F, H, W, with_truth=with_truth).update(xt[:, cut:], None if yyt is None else yyt[cut:])
        before = b.tables()
        assert a.merge(b) is a and a.n_times == T
        worst = R.check_merge(x[:, :cut], None if yy is None else yy[:cut], x[:, cut:], None if yy is None else yy[cut:], _state(a.tables()), range(H * W))
        print(f"{kind} ({route}, truth {with_truth}): worst fraction of the merge bound {worst:.4f}")
        one = R.comoments(x, yy)
        assert np.array_equal(one["n"], a.tables().n.numpy().reshape(one["n"].shape)) and np.array_equal(one["invalid"], a.tables().invalid.numpy())
        assert torch.equal(b.tables().sums, before.sums) and torch.equal(b.tables().n, before.n)   # the other is left alone


def test_merge_into_an_empty_accumulator_is_bit_identical(route):
    x, y, xt, yt = _fields("nan_hours", 2, 9, 3, 2, 4, seed=6)
    full = DP.DependenceAccumulator(2, 3, 2, 4).update(xt, yt)
    empty = DP.DependenceAccumulator(2, 3, 2, 4).merge(full)
    assert _same(R.comoments(x, y), empty.tables())
    again = DP.DependenceAccumulator(2, 3, 2, 4).update(xt, yt).merge(DP.DependenceAccumulator(2, 3, 2, 4))   # and an empty one merged in
    assert _same(R.comoments(x, y), again.tables())


# ------------------------------------------------------------------------------------------------------------------ refusals of the module

def test_what_the_module_refuses():
    x, y, xt, yt = _fields("smooth", 2, 6, 2, 2, 4)
    A = DP.DependenceAccumulator
    acc = A(2, 2, 2, 4)
    for call, text in ((lambda: acc.update(xt), "made with a truth"), (lambda: A(2, 2, 2, 4, with_truth=False).update(xt, yt), "made without a truth"),
                       (lambda: acc.update(xt, yt[:5]), r"must be \(M >= 1,\) \+ truth"), (lambda: acc.update(xt.long(), yt.long()), "must be floating point"),
                       (lambda: acc.update(xt[:1], yt), r"must be \(M, T, F, H, W\) = \(2, T, 2, 2, 4\)"),
                       (lambda: A(2, 2, 2, 4, with_truth=False).update(xt.long()), r"must be floating point \(M, T, F, H, W\)"),
                       (lambda: A(0, 2, 2, 4), "M 0 must be an integer >= 1"), (lambda: DP.comoments(xt[0], yt), r"must be \(M, T, F, H, W\)"),
                       (lambda: acc.merge(A(3, 2, 2, 4)), "the other accumulator is"), (lambda: acc.merge(A(2, 2, 2, 4, with_truth=False)), "the other accumulator is"),
                       (lambda: DP.truth_statistics(DP.comoments(xt)), "needs tables with a truth"), (lambda: DP.taylor(DP.comoments(xt)), "needs tables with a truth"),
                       (lambda: DP.correlation_error(DP.comoments(xt)), "needs tables with a truth"),
                       (lambda: DP.dependence_report(xt, yt, names=["a"]), "1 names for 2 variables")):
        with pytest.raises(ValueError, match=text):
            call()


# ------------------------------------------------------------------------------------------------------------------ statistics

def test_covariance_and_means_agree_with_numpy(route):
    M, T, F, H, W = 2, 40, 3, 2, 4
    x, y, xt, yt = _fields("smooth", M, T, F, H, W, seed=9)
    t = DP.comoments(xt, yt)
    rows = np.concatenate([y[None], x]).astype(np.float64)                       # (D, T, F, hw)
    cov, mean, corr = DP.covariance(t, ddof=1).numpy().reshape(M + 1, F, F, -1), DP.means(t).numpy().reshape(M + 1, F, -1), DP.correlation(t).numpy()
    for d in range(M + 1):
        for c in range(H * W):
            want = np.cov(rows[d, :, :, c].T)
            assert np.allclose(cov[d, :, :, c], want, rtol=1e-12, atol=1e-12 * np.abs(want).max()), (d, c)
            assert np.allclose(mean[d, :, c], rows[d, :, :, c].mean(axis=0), rtol=1e-12, atol=1e-13)
            assert np.allclose(corr.reshape(M + 1, F, F, -1)[d, :, :, c], np.corrcoef(rows[d, :, :, c].T), rtol=1e-12, atol=1e-12)
    assert tuple(DP.covariance(t).shape) == (M + 1, F, F, H, W) and tuple(DP.means(t).shape) == (M + 1, F, H, W)
    assert np.allclose(DP.covariance(t).numpy() * T / (T - 1), DP.covariance(t, ddof=1).numpy(), rtol=1e-14)


def test_a_linear_relation_with_a_power_of_two_slope_has_correlation_one(route):
    """v = a u + b with a = -4 and small integers: every e_v = a e_u exactly, so C_uv = a C_uu and the quotient is exact"""
    rng = np.random.default_rng(0)
    u = rng.integers(-50, 50, (1, 30, 1, 8)).astype(np.float32)
    xt = torch.from_numpy(np.concatenate([u, -4.0 * u + 3.0, 0.5 * u - 7.0], axis=2)).view(1, 30, 3, 2, 4)
    t = DP.comoments(xt)
    corr = DP.correlation(t)[0]
    want = torch.tensor([[1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, 1.0]], dtype=torch.float64).view(3, 3, 1, 1).expand(3, 3, 2, 4)
    assert float((corr - want).abs().max()) <= 2.0 ** -52
    assert float((DP.pooled_correlation(t)[0] - want[:, :, 0, 0]).abs().max()) <= 2.0 ** -52


def test_a_constant_series_has_zero_variance_and_no_correlation(route):
    x, y, xt, yt = _fields("constant", 2, 10, 2, 1, 4)
    t = DP.comoments(xt, yt)
    assert float(DP.covariance(t).abs().max()) == 0.0 and bool(torch.isnan(DP.correlation(t)).all())
    s = DP.truth_statistics(t)
    assert float(s.mean_bias.abs().max()) == 0.0 and float(s.centred_rmse.abs().max()) == 0.0
    assert bool(torch.isnan(s.std_ratio).all()) and bool(torch.isnan(s.correlation).all()) and bool(torch.isnan(DP.pooled_correlation(t)).all())
    one = DP.comoments(xt[:, :1], yt[:1])   # n = 1
    assert bool(torch.isnan(DP.correlation(one)).all()) and float(DP.means(one)[0, 0, 0, 0]) == 2.5


def test_a_member_equal_to_the_truth(route):
    x, y, xt, yt = _fields("nan_hours", 1, 30, 2, 2, 4, seed=2)
    t = DP.comoments(yt[None].expand(3, -1, -1, -1, -1), yt)
    s = DP.truth_statistics(t)
    ok = t.n[1:, None].expand_as(s.mean_bias) >= 2
    assert bool(ok.any())
    assert float(s.mean_bias[ok].abs().max()) == 0.0 and float(s.centred_rmse[ok].abs().max()) == 0.0
    assert s.std_ratio[ok].unique().tolist() == [1.0] and s.correlation[ok].unique().tolist() == [1.0]
    ty = DP.taylor(t)
    assert tuple(ty.shape) == (3, 2, 3) and ty[..., 0].unique().tolist() == [1.0] and ty[..., 1].unique().tolist() == [1.0] and float(ty[..., 2].abs().max()) == 0.0
    bias, rmse, cells = DP.correlation_error(t)
    assert float(bias.abs().max()) == 0.0 and float(rmse.abs().max()) == 0.0 and cells.dtype == torch.int64 and tuple(cells.shape) == (3, 2, 2)


def test_independent_fields_have_a_small_pooled_correlation(route):
    """``smooth`` random walks are strongly autocorrelated, so white noise is the field: variables of one draw and members of two
    seeds are independent standard normals, 200 hours on 16 cells.  The pooled correlation of N = 3200 independent pairs has standard
    deviation 1 / sqrt(N) = 0.018; the margin is 5 of them, 0.09 (seen on the CPU: below 0.04)."""
    rng = np.random.default_rng(11)
    xt = torch.from_numpy(rng.standard_normal((2, 200, 2, 4, 4)).astype(np.float32))
    yt = torch.from_numpy(np.random.default_rng(12).standard_normal((200, 2, 4, 4)).astype(np.float32))
    t = DP.comoments(xt, yt)
    pooled = DP.pooled_correlation(t)
    assert tuple(pooled.shape) == (3, 2, 2) and float(pooled[:, 0, 1].abs().max()) < 0.09 and float((pooled[:, 0, 0] - 1).abs().max()) < 1e-15
    assert float(DP.taylor(t)[..., 1].abs().max()) < 0.09
    print("pooled |corr|:", float(pooled[:, 0, 1].abs().max()), float(DP.taylor(t)[..., 1].abs().max()))


def test_the_centred_rmse_obeys_the_taylor_identity_against_numpy(route):
    M, T, F, H, W = 2, 25, 2, 1, 4
    x, y, xt, yt = _fields("smooth", M, T, F, H, W, seed=13)
    s = DP.truth_statistics(DP.comoments(xt, yt))
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    ex, ey = xd - xd.mean(axis=1, keepdims=True), yd - yd.mean(axis=0, keepdims=True)
    assert np.allclose(s.centred_rmse.numpy().reshape(M, F, -1), np.sqrt(((ex - ey[None]) ** 2).mean(axis=1)), rtol=1e-12)
    assert np.allclose(s.mean_bias.numpy().reshape(M, F, -1), (xd - yd[None]).mean(axis=1), rtol=1e-12, atol=1e-14)
    assert np.allclose(s.std_ratio.numpy().reshape(M, F, -1), xd.std(axis=1) / yd.std(axis=0)[None], rtol=1e-12)


def test_the_reports_keys_and_shapes(route):
    M, T, F, H, W = 3, 20, 3, 2, 4
    x, y, xt, yt = _fields("nan_hours", M, T, F, H, W, seed=14)
    rep = DP.dependence_report(xt, yt, names=["u", "v", "p"])
    assert isinstance(rep, VariableReport) and rep.names == ["u", "v", "p"]
    shapes = dict(mean_bias=(M,), std_ratio=(M,), correlation=(M,), centred_rmse=(M,), mean_bias_map=(M, H, W), std_ratio_map=(M, H, W),
                  correlation_map=(M, H, W), centred_rmse_map=(M, H, W), pair_correlation_truth=(F,), pair_correlation=(M, F), pair_error_bias=(M, F),
                  pair_error_rmse=(M, F), pair_error_cells=(M, F), invalid=(M + 1,))
    for name, v in rep:
        assert set(v) == set(shapes)
        for key, shape in shapes.items():
            assert tuple(v[key].shape) == shape, (name, key)
            assert v[key].dtype == (torch.int64 if key in ("pair_error_cells", "invalid") else torch.float64), key
    flat = rep.as_dict()
    want = {f"dependence/{n}/{k}{s}" for n in rep.names for k in ("mean_bias", "std_ratio", "correlation", "centred_rmse") for s in ("", "_std")}
    want |= {f"dependence/{n}/corr_{o}{s}" for n in rep.names for o in rep.names if o != n for s in ("", "_std", "_error", "_error_std", "_truth")}
    assert set(flat) == want and all(isinstance(v, float) for v in flat.values())
    assert flat["dependence/u/corr_v_truth"] == pytest.approx(float(rep["u"]["pair_correlation_truth"][1]))
    assert DP.DependenceReport([], []).as_dict() == {}


# ------------------------------------------------------------------------------------------------------------------ refusals of the launcher

BAD_ARG, BAD_SHAPE, UNSUPPORTED = -1, -2, -3
DEV = object()   # a made-up device address: argument number i of a call is 4096 (16 + i); nothing dereferences it
M20 = 1 << 20
BASE = dict(x=DEV, y=DEV, n=DEV, pivot=DEV, truth_pivot=DEV, sums=DEV, invalid=DEV, M=2, T=4, F=2, hw=16, stream=None)
REFUSED = ([(f"{n} null", {n: None}, BAD_ARG) for n in ("x", "n", "pivot", "truth_pivot", "sums", "invalid")]
           + [(f"{n} off by 4", {n: 4}, BAD_ARG) for n in ("x", "y", "n", "pivot", "truth_pivot", "sums", "invalid")]
           + [("sums off by 8", dict(sums=8), BAD_ARG), ("hw = 6", dict(hw=6), UNSUPPORTED), ("hw = 0", dict(hw=0), UNSUPPORTED),
              ("F = 0", dict(F=0), UNSUPPORTED), ("F = 9", dict(F=9), UNSUPPORTED), ("no member", dict(M=0), UNSUPPORTED), ("T < 0", dict(T=-1), BAD_ARG),
              ("T over 2^20", dict(T=M20 + 1), BAD_SHAPE), ("grid", dict(M=0x7FFFFFFE, hw=1 << 12), BAD_SHAPE)])


def _arguments(change):
    """the base call, which would be valid and is never made, with `change` applied"""
    assert change and set(change) <= set(BASE)
    out = []
    for i, (arg, value) in enumerate(BASE.items()):
        address = 4096 * (16 + i)
        if arg in change:
            c = change[arg]
            value = address + c if value is DEV and isinstance(c, int) else c
        elif value is DEV:
            value = address
        out.append(value)
    return out


def test_the_launcher_refuses_out_of_range_arguments_before_any_launch():
    assert all(code < 0 and len(_arguments(change)) == len(_lib._PROTOS["c2w_comoments_update"]) for _, change, code in REFUSED)
    if torch.cuda.is_available():
        pytest.skip("made-up device addresses: only where nothing can launch")
    build.build(verbose=False)
    lib = _lib.load()
    wrong = [(what, rc, code) for what, change, code in REFUSED for rc in [lib.c2w_comoments_update(*_arguments(change))] if rc != code]
    assert not wrong, wrong
    assert lib.c2w_comoments_update(*_arguments(dict(T=0))) == 0   # T = 0 returns 0 and writes nothing
    assert lib.c2w_comoments_supported(16, 8) == 1 and lib.c2w_comoments_supported(6, 2) == 0 and lib.c2w_comoments_supported(16, 9) == 0


# ------------------------------------------------------------------------------------------------------------------ the host program

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_comoments(request, tmp_path_factory):
    """a stand-alone program, once plain and once under the address and undefined-behaviour sanitizers; it is run directly, never loaded
    into Python"""
    return host_program.build(tmp_path_factory, "comoments", sanitize=request.param == "sanitized", fp_contract_off=True, timeout=900)


@pytest.mark.parametrize("M,T,F,hw,has_truth", [(1, 1, 1, 4, 0), (2, 9, 1, 1028, 1), (1, 4, 2, 516, 1), (2, 5, 3, 260, 0), (1, 14, 4, 1028, 1),
                                                (1, 3, 5, 256, 1), (1, 6, 6, 12, 0), (1, 7, 7, 264, 1), (2, 8, 8, 260, 1)])
def test_every_cell_hour_is_read_once_and_every_state_entry_loaded_and_stored_once(host_comoments, M, T, F, hw, has_truth):
    """one thread, a chunk and a thread, exactly one chunk, five chunks; T around the unroll; every cells-per-thread"""
    rc = subprocess.run([str(host_comoments), "visit"] + [str(a) for a in (M, T, F, hw, has_truth)], timeout=600).returncode
    assert rc == 0, f"check {rc} of host_comoments_main.cpp failed"


@pytest.mark.parametrize("F", range(1, 9))
def test_the_host_program_equals_the_reference_and_the_emulation(host_comoments, tmp_path, F):
    """csrc/comoments_maps.h compiled for the host: every kind in turn; on 8 cells every cut of T = 6 into calls held against the
    single call inside the program, on a ragged second chunk one cut; the program's own straight-line restatement, the NumPy
    reference and the emulation of the launcher all give the same bits"""
    M, T = 2, 6
    chunk = emu_comoment_ops.chunk_cells(F)
    for i, kind in enumerate(R.KINDS):
        ragged = (i + F) % 4 == 0
        hw, has_truth = (chunk + 4 if ragged else 8), (i + F) % 2
        x, y = R.field(kind, (M, T, F, hw), i), R.field(kind, (T, F, hw), i + 50)
        files = [str(tmp_path / n) for n in ("x.f32", "y.f32", "n.i32", "pivot.f32", "tpivot.f32", "sums.f64", "invalid.i64")]
        x.tofile(files[0]), y.tofile(files[1])
        args = [str(a) for a in (M, T, F, hw, has_truth, 0b01010 if ragged else -1)]
        rc = subprocess.run([str(host_comoments), "update"] + args + files, timeout=600).returncode
        assert rc == 0, (kind, rc)
        D = M + has_truth
        got = [np.fromfile(p, dt) for p, dt in zip(files[2:], (np.int32, np.float32, np.float32, np.float64, np.int64))]
        assert R.same_bits(R.comoments(x, y if has_truth else None), *got), kind
        st = DP.DependenceAccumulator(M, F, 1, hw, with_truth=bool(has_truth))
        assert emu_comoment_ops.comoments_update(torch.from_numpy(x), torch.from_numpy(y) if has_truth else None, st.n, st.pivot, st.truth_pivot, st.sums,
                                                 st.invalid, M, T, F, hw)
        assert R.same_bits(_state(st.tables()), *got), kind


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_comoments_supported": "int", "c2w_comoments_update": "int"}
    c_abi.assert_declared(names, "comoments.hip", dependence_ops, ("supported", "comoments_update"))
