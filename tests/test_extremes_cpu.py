"""Extremes of an ensemble without a GPU (climate2weather_amd/extremes.py, csrc/extremes_maps.h): the block extremes of both routes --
the torch definition and the emulation of the launchers standing in for the library -- against plain loops over keys, bit for bit and
for every cut of the time axis; the L-moments against rational arithmetic within the bound extremes_maps.h derives; the GEV fit
against the closed-form population L-moments and scipy; known answers; what the launchers refuse; and the header compiled for the
host as a program of its own, plain and under the sanitizers."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import c_abi
import emu_extreme_ops
import fp64_extremes_ref as R
import host_program
from climate2weather_amd import _lib, build, extreme_ops
from climate2weather_amd import extremes as EX
from climate2weather_amd.ensemble_host import VariableReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64)


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of extremes.py on CPU tensors"""
    if request.param == "launcher":
        emu_extreme_ops.install(monkeypatch, extreme_ops, EX)
    return request.param


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int32).numpy().view(np.uint32)


def _fields(kind, M, T, F, H, W, seed=0, block=3):
    x = R.field(kind, (M, T, F, H * W), seed, block)
    y = R.field(kind, (T, F, H * W), seed + 1, block)
    return x, y, torch.from_numpy(x).view(M, T, F, H, W), torch.from_numpy(y).view(T, F, H, W)


def _directions(F, which):
    return [("max", "min")[f % 2] for f in range(F)] if which == "mixed" else [which] * F


# ------------------------------------------------------------------------------------------------------------------ block extremes

@pytest.mark.parametrize("which", ["max", "min", "mixed"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_the_block_extremes_equal_the_reference_bit_for_bit(route, kind, which):
    M, T, F, H, W, block = 2, 7, 2, 2, 4, 3
    x, y, xt, yt = _fields(kind, M, T, F, H, W)
    dirs = _directions(F, which)
    for partial in ("drop", "keep"):
        want, invalid = R.block_extremes(x, y, block, [d == "max" for d in dirs], partial == "keep")
        t = EX.block_extremes(xt, yt, block, dirs if which == "mixed" else which, partial)
        assert t.n_blocks == want.shape[2] and t.open_hours == T % block and tuple(t.extremes.shape) == (M + 1, F, want.shape[2], H, W)
        assert np.array_equal(_bits(t.extremes).reshape(want.shape), want), (kind, partial)
        assert np.array_equal(t.invalid.numpy(), invalid)
    if route == "launcher":
        assert emu_extreme_ops.CALLS and emu_extreme_ops.CALLS[0][0] == "update"


@pytest.mark.parametrize("block", [3, 1, 8])
def test_every_cut_of_the_time_axis_gives_the_same_bits(route, block):
    """T = 7: all 64 ways to cut it into calls; block 3 (two blocks and an open hour), 1 and one longer than the run"""
    M, T, F, H, W = 1, 7, 2, 1, 4
    x, y, xt, yt = _fields("nan_hours", M, T, F, H, W, seed=3, block=block)
    dirs = _directions(F, "mixed")
    want = {p: R.block_extremes(x, y, block, [d == "max" for d in dirs], p == "keep") for p in ("drop", "keep")}
    for cuts in range(1 << (T - 1)):
        acc = EX.ExtremeAccumulator(M, F, H, W, block, dirs, max_blocks=max(1, T // block))
        a = 0
        for t in range(1, T + 1):
            if t == T or (cuts >> (t - 1)) & 1:
                acc.update(xt[:, a:t], yt[a:t])
                a = t
        for p in ("drop", "keep"):
            t = acc.tables(p)
            assert np.array_equal(_bits(t.extremes).reshape(want[p][0].shape), want[p][0]), (cuts, p)
            assert np.array_equal(t.invalid.numpy(), want[p][1]), cuts
        assert acc.tables().open_hours == T % block


def test_without_a_truth_and_with_an_empty_update(route):
    x, y, xt, yt = _fields("smooth", 2, 6, 1, 1, 4)
    acc = EX.ExtremeAccumulator(2, 1, 1, 4, 2, "min", with_truth=False, max_blocks=3)
    acc.update(xt[:, :0]).update(xt)
    want, invalid = R.block_extremes(x, None, 2, [False])
    assert np.array_equal(_bits(acc.tables().extremes).reshape(want.shape), want) and np.array_equal(acc.tables().invalid.numpy(), invalid)


def test_an_update_longer_than_one_launch_takes_is_walked_in_parts(route, monkeypatch):
    monkeypatch.setattr(EX, "MAX_CALL", 2)
    x, y, xt, yt = _fields("nan_hours", 2, 7, 2, 1, 4, seed=8)
    t = EX.block_extremes(xt, yt, 3, ["min", "max"], "keep")
    want, invalid = R.block_extremes(x, y, 3, [False, True], True)
    assert np.array_equal(_bits(t.extremes).reshape(want.shape), want) and np.array_equal(t.invalid.numpy(), invalid)
    if route == "launcher":
        assert [c[2] for c in emu_extreme_ops.CALLS] == [2, 2, 2, 1] and [c[7] for c in emu_extreme_ops.CALLS] == [0, 2, 4, 6]


def test_tables_works_on_a_copy_and_the_state_dict_round_trip(route):
    M, T, F, H, W, block = 2, 7, 2, 1, 4, 3
    x, y, xt, yt = _fields("inf", M, T, F, H, W)
    acc = EX.ExtremeAccumulator(M, F, H, W, block, "max", max_blocks=4).update(xt[:, :4], yt[:4])
    t = acc.tables("keep")
    t.extremes.fill_(0.0), t.invalid.fill_(-1)
    sd = acc.state_dict()
    acc.update(xt[:, 4:], yt[4:])
    other = EX.ExtremeAccumulator(M, F, H, W, block, "max", max_blocks=4).load_state_dict(sd).update(xt[:, 4:], yt[4:])
    want, invalid = R.block_extremes(x, y, block, [True] * F, True)
    for a in (acc, other):
        assert np.array_equal(_bits(a.tables("keep").extremes).reshape(want.shape), want) and np.array_equal(a.tables().invalid.numpy(), invalid)


def test_strided_and_half_precision_inputs(route):
    x, y, xt, yt = _fields("smooth", 2, 6, 2, 2, 4)
    big = torch.zeros((2, 6, 2, 2, 8))
    big[..., ::2] = xt
    a, b = EX.block_extremes(big[..., ::2], yt, 3, "max"), EX.block_extremes(xt, yt, 3, "max")
    assert torch.equal(a.extremes, b.extremes)
    h = EX.block_extremes(xt.half(), yt.half(), 3, "max")
    assert torch.equal(h.extremes, EX.block_extremes(xt.half().float(), yt.half().float(), 3, "max").extremes)


def test_an_unsupported_shape_takes_the_general_route(monkeypatch):
    emu_extreme_ops.install(monkeypatch, extreme_ops, EX)
    x, y, xt, yt = _fields("smooth", 1, 6, 1, 2, 3)   # hw = 6
    t = EX.block_extremes(xt, yt, 3, "max")
    want, _ = R.block_extremes(x, y, 3, [True])
    assert np.array_equal(_bits(t.extremes).reshape(want.shape), want)
    lm, nv = EX.lmoments(t.extremes)
    assert [c[0] for c in emu_extreme_ops.CALLS] == [] and tuple(lm.shape) == (2, 1, 4, 2, 3)   # the launchers were asked "supported" only
    R.check_lmoments(_np32(t.extremes).reshape(2, 2, 6), lm.numpy().reshape(2, 4, 6), nv.numpy().reshape(2, 6))


def test_the_emulation_restates_the_constants_of_the_kernel():
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "extremes_maps.h")).read()
    for text in ("THREADS = 256", "CELLS = 4", "CHUNK = THREADS * CELLS", "UNROLL = 8", "MAX_BLOCK = 1 << 20, MAX_B = 4096, MAX_T = 1 << 20, MAX_N = 64",
                 "NONE = 0u", "NAN_BITS = 0x7FC00000u", "hw >= 4 && hw % 4 == 0 && block >= 1 && block <= MAX_BLOCK && B >= 1 && B <= MAX_B",
                 "hw >= 4 && hw % 4 == 0 && n >= 1 && n <= MAX_N", "r == 1 ? 1 : r == 2 ? 3 : r == 3 ? 13 : 63", "r == 1 ? 1 : r == 2 ? 4 : r == 3 ? 38 : 240"):
        assert text in core, text
    e = emu_extreme_ops
    assert (e.THREADS, e.CELLS, e.CHUNK, e.MAX_BLOCK, e.MAX_B, e.MAX_T, e.MAX_N, e.NONE, e.NAN_BITS) == (256, 4, 1024, 1 << 20, 4096, 1 << 20, 64, 0, 0x7FC00000)
    assert EX.MAX_CALL == e.MAX_T and EX.NAN_BITS == e.NAN_BITS == R.NAN_BITS and (R.W, R.Q) == ((1, 3, 13, 63), (1, 4, 38, 240))
    assert '#include "core_side.h"' in core and not any(f"#define C2W_{side}" in core for side in ("HD", "BOTH", "CORE_HOST"))


# ------------------------------------------------------------------------------------------------------------------ L-moments

def _np32(t):
    return t.contiguous().numpy().astype(np.float32)


def _table(kind, Rr, n, hw, seed, nan_share=0.0):
    t = R.field(kind, (Rr, n, 1, hw), seed).reshape(Rr, n, hw)
    if nan_share:
        t = np.where(np.random.default_rng(seed + 7).random(t.shape) < nan_share, np.float32(np.nan), t).astype(np.float32)
    return t


@pytest.mark.parametrize("n", NS)
def test_the_lmoments_lie_within_the_derived_bound(route, n):
    worst = 0.0
    for kind, nan_share in (("smooth", 0.0), ("pressure", 0.0), ("denormal", 0.0), ("constant", 0.0), ("pressure", 0.3)):
        t = _table(kind, 2, n, 8, seed=n, nan_share=nan_share)
        lm, nv = EX.lmoments(torch.from_numpy(t).view(2, n, 2, 4))
        assert lm.dtype == torch.float64 and nv.dtype == torch.int32 and tuple(lm.shape) == (2, 4, 2, 4) and tuple(nv.shape) == (2, 2, 4)
        worst = max(worst, R.check_lmoments(t, lm.numpy().reshape(2, 4, 8), nv.numpy().reshape(2, 8)))
    print(f"n = {n} ({route}): worst fraction of the bound {worst:.3f}")
    if route == "launcher":
        assert ("lmoments", 2, n, 8) in emu_extreme_ops.CALLS


def test_more_than_64_blocks_take_the_general_route(route):
    t = _table("pressure", 1, 120, 4, seed=5)
    lm, nv = EX.lmoments(torch.from_numpy(t).view(1, 120, 1, 4))
    R.check_lmoments(t, lm.numpy().reshape(1, 4, 4), nv.numpy().reshape(1, 4))


def test_nans_that_leave_fewer_than_four_values_give_nan_in_exactly_those_orders(route):
    t = _table("smooth", 1, 5, 8, seed=2)
    for c, keep in enumerate((5, 4, 3, 2, 1, 0, 4, 3)):
        t[0, keep:, c] = np.nan
    lm, nv = EX.lmoments(torch.from_numpy(t).view(1, 5, 2, 4))
    lm, nv = lm.numpy().reshape(4, 8), nv.numpy().reshape(8)
    assert nv.tolist() == [5, 4, 3, 2, 1, 0, 4, 3]
    assert np.array_equal(np.isnan(lm), np.array([[k < r + 1 for k in nv] for r in range(4)]))
    R.check_lmoments(t, lm.reshape(1, 4, 8), nv.reshape(1, 8))


def test_scipy_agrees(route):
    """a sanity check of the definition: scipy's own error against the rational reference, times 4, is the tolerance"""
    from scipy import stats
    t = _table("pressure", 1, 12, 8, seed=11)
    lm = EX.lmoments(torch.from_numpy(t).view(1, 12, 2, 4))[0].numpy().reshape(4, 8)
    sc = stats.lmoment(t[0].astype(np.float64), order=[1, 2, 3, 4], axis=0, standardize=False)
    for o in range(4):
        exact = [R.lmoments_exact(t[0, :, c])[0][o] for c in range(8)]
        tol = 4 * max(abs(Fraction(float(sc[o, c])) - exact[c]) for c in range(8))
        assert tol > 0 and all(abs(Fraction(float(lm[o, c])) - Fraction(float(sc[o, c]))) <= tol for c in range(8)), (o, float(tol))


def test_the_unpivoted_formula_misses_the_bound_on_a_pressure_field():
    """the reason for the pivot: the same sums on the unreduced values, in float64, are outside the bound -- on extremes at 101325 Pa
    that differ by 5 Pa by up to 200 times (at the 1e5 +- 1e3 of the "pressure" kind the unreduced sums stay inside it: up to 0.64 of
    the bound was seen; the bound is a worst case and scales with the spread, the error of the unreduced sums with the level)"""
    t = (np.float32(101325) + np.float32(5) * np.random.default_rng(4).standard_normal((1, 64, 32)).astype(np.float32)).astype(np.float32)
    s = np.sort(t[0].astype(np.float64), axis=0)
    n, j = 64, np.arange(64, dtype=np.float64)[:, None]
    b = [np.zeros(32) for _ in range(4)]
    for r, num in enumerate((np.ones_like(j), j, j * (j - 1), j * (j - 1) * (j - 2))):
        for i in range(n):
            b[r] = b[r] + num[i] * s[i]
        b[r] = b[r] / float(math.prod(n - i for i in range(r + 1)))
    naive = [b[0], 2 * b[1] - b[0], 6 * b[2] - 6 * b[1] + b[0], 20 * b[3] - 30 * b[2] + 12 * b[1] - b[0]]
    missed = 0
    for c in range(32):
        l, nv, A = R.lmoments_exact(t[0, :, c])
        missed += sum(abs(Fraction(float(naive[o][c])) - l[o]) > R.lmoment_bound(o + 1, nv, A, l[0]) for o in (1, 2, 3))
    assert missed > 0
    lm, nv = EX.lmoments(torch.from_numpy(t).view(1, 64, 4, 8))
    R.check_lmoments(t, lm.numpy().reshape(1, 4, 32), nv.numpy().reshape(1, 32))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 12, 64])
def test_the_series_0_to_n_minus_1_has_its_known_moments(route, n):
    """l1 = (n - 1) / 2 exactly; l2 = (n + 1) / 6 is no binary fraction and l3 = l4 = 0 are differences of rounded quotients, so
    these three are held to the derived bound around the known rational values -- an exact 0 wherever the quotients round alike"""
    t = torch.arange(n, dtype=torch.float32).flip(0).view(n, 1, 1).expand(n, 1, 4).contiguous()
    lm = EX.lmoments(t)[0][:, 0, 0].tolist()
    want = [Fraction(n - 1, 2), Fraction(n + 1, 6), Fraction(0), Fraction(0)]
    A = sum(abs(Fraction(j - n // 2)) for j in range(n))
    for r in range(4):
        if n < r + 1:
            assert math.isnan(lm[r])
        elif r == 0:
            assert lm[0] == (n - 1) / 2
        else:
            assert abs(Fraction(lm[r]) - want[r]) <= R.lmoment_bound(r + 1, n, A, want[0]), (n, r, lm[r])
    if n in (3, 4, 7):
        assert lm[2] == 0.0   # 6 b2 and 6 b1 are the same number here


def test_the_plane_wise_reference_of_the_gpu_tier_equals_the_loops():
    for i, kind in enumerate(R.KINDS):
        x, y = R.field(kind, (2, 7, 2, 8), i), R.field(kind, (7, 2, 8), i + 20)
        for partial in (False, True):
            a, b = R.block_extremes(x, y, 3, [True, False], partial), R.block_extremes_by_planes(x, y, 3, [True, False], partial)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), kind


# ------------------------------------------------------------------------------------------------------------------ the GEV

KS = [i * 0.05 for i in range(-18, 61)]   # -0.9 .. 3, 0 exactly
XI, ALPHA = 3.0, 2.0


def _population(ks, xi=XI, alpha=ALPHA):
    L = np.array([R.gev_population_lmoments(xi, alpha, k) + (0.0,) for k in ks])           # (n, 4)
    return torch.from_numpy(np.ascontiguousarray(L.T)).view(4, 1, len(ks))


def test_the_fit_recovers_the_parameters_from_the_population_lmoments():
    assert KS[18] == 0.0
    xi, alpha, k, unfitted = EX.gev_fit(_population(KS))
    assert int(unfitted) == 0
    assert float((k.view(-1) - torch.tensor(KS, dtype=torch.float64)).abs().max()) <= 1e-9
    assert float((alpha / ALPHA - 1).abs().max()) <= 1e-9 and float((xi / XI - 1).abs().max()) <= 1e-9


def test_the_return_levels_equal_scipy():
    from scipy import stats
    periods = [2, 5, 10, 20, 100, 1000]
    xi, alpha, k, _ = EX.gev_fit(_population(KS))
    levels = EX.gev_return_level(xi, alpha, k, periods).view(len(periods), len(KS)).numpy()
    want = np.stack([stats.genextreme.ppf(1.0 - 1.0 / p, np.array(KS), XI, ALPHA) for p in periods])
    assert np.abs(levels / want - 1).max() <= 1e-10
    gumbel = np.array([stats.gumbel_r.ppf(1.0 - 1.0 / p, XI, ALPHA) for p in periods])
    assert np.abs(levels[:, 18] / gumbel - 1).max() <= 1e-10
    exact = EX.gev_return_level(torch.full((1, 1), XI), torch.full((1, 1), ALPHA), torch.zeros((1, 1)), periods).view(-1).numpy()
    assert np.abs(exact / gumbel - 1).max() <= 1e-13


def test_the_fit_and_the_levels_are_continuous_across_zero():
    """k = -1e-9, 0, 1e-9: the fit recovers each, and the levels move by no more than their first-order term |k| alpha ln(-ln p)^2
    (twice the Taylor coefficient) -- a form that is 0/0 at zero would jump by far more"""
    ks, periods = [-1e-9, 0.0, 1e-9], [2, 10, 100, 1000]
    xi, alpha, k, unfitted = EX.gev_fit(_population(ks))
    assert int(unfitted) == 0 and float((k.view(-1) - torch.tensor(ks, dtype=torch.float64)).abs().max()) <= 1e-9
    assert float((alpha / ALPHA - 1).abs().max()) <= 1e-9 and float((xi / XI - 1).abs().max()) <= 1e-9
    one = lambda v: torch.full((1, 1), v, dtype=torch.float64)
    lv = [EX.gev_return_level(one(XI), one(ALPHA), one(kv), periods).view(-1) for kv in ks]
    for i, p in enumerate(periods):
        step = 1e-9 * ALPHA * math.log(-math.log1p(-1.0 / p)) ** 2
        assert 0 < abs(float(lv[0][i] - lv[1][i])) <= step and 0 < abs(float(lv[2][i] - lv[1][i])) <= step, p
    x = torch.tensor([1.0, 3.0, 9.0], dtype=torch.float64).view(3, 1)
    cdf = [EX.gev_cdf(x, one(XI).view(1, 1), one(ALPHA).view(1, 1), one(kv).view(1, 1)).view(-1) for kv in ks]
    assert float((cdf[0] - cdf[1]).abs().max()) <= 1e-8 and float((cdf[2] - cdf[1]).abs().max()) <= 1e-8


def test_the_cdf_inverts_the_return_level_and_is_0_or_1_outside_the_support():
    from scipy import stats
    ks = torch.tensor([-0.4, 0.0, 0.3, 1.5], dtype=torch.float64).view(1, 4)
    xi, alpha = torch.full_like(ks, XI), torch.full_like(ks, ALPHA)
    levels = EX.gev_return_level(xi, alpha, ks, [2, 20, 200])                               # (3, 1, 4)
    p = EX.gev_cdf(levels, xi, alpha, ks)
    assert float((p - torch.tensor([0.5, 0.95, 0.995], dtype=torch.float64).view(3, 1, 1)).abs().max()) <= 1e-14
    x = torch.tensor([-100.0, 0.0, 4.0, 100.0], dtype=torch.float64).view(4, 1, 1)
    got = EX.gev_cdf(x, xi, alpha, ks).view(4, 4).numpy()
    want = stats.genextreme.cdf(x.view(4, 1).numpy(), ks.view(1, 4).numpy(), XI, ALPHA)
    assert np.abs(got - want).max() <= 1e-14 and got[0, 0] == 0.0 and got[3, 2] == 1.0 and got[3, 3] == 1.0
    assert math.isnan(float(EX.gev_cdf(torch.tensor([[float("nan")]]), xi[:, :1], alpha[:, :1], ks[:, :1])))


def test_unfitted_counts_exactly_the_constant_the_two_block_and_the_degenerate_cells():
    ext = torch.tensor(R.field("smooth", (1, 6, 1, 8), 1).reshape(1, 1, 6, 2, 4))
    ext[0, 0, :, 0, 0] = 4.0                                    # constant: l2 = 0
    ext[0, 0, 2:, 0, 1] = float("nan")                          # two blocks: l3 is NaN
    ext[0, 0, :, 0, 2] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 1.0])   # t3 = 1: x_(j) = [j = n - 1]
    lm, nv = EX.lmoments(ext)
    t3 = EX.lmoment_ratios(lm)[1]
    assert float(t3[0, 0, 0, 2]) == 1.0 and int(nv[0, 0, 0, 1]) == 2
    xi, alpha, k, unfitted = EX.gev_fit(lm)
    assert unfitted.tolist() == [[3]] and tuple(unfitted.shape) == (1, 1)
    bad = torch.isnan(xi) & torch.isnan(alpha) & torch.isnan(k)
    assert bad.view(-1).tolist() == [True, True, True] + [False] * 5 and bool(torch.isfinite(xi.view(-1)[3:]).all())


# ------------------------------------------------------------------------------------------------------------------ the algebra, the report

def test_identical_members_have_zero_errors(route):
    _, _, xt, yt = _fields("smooth", 1, 40, 2, 2, 4, seed=9)
    samples = yt[None].expand(3, -1, -1, -1, -1).contiguous()
    t = EX.block_extremes(samples, yt, 5, ["max", "min"])
    lm, nv = EX.lmoments(t.extremes)
    xi, alpha, k, unfitted = EX.gev_fit(lm)
    levels = EX.gev_return_level(xi, alpha, k, [2, 10])
    for a in EX.mean_extreme_error(lm) + EX.lmoment_ratio_error(lm) + EX.return_level_error(levels)[:2]:
        assert float(a.abs().max()) == 0.0
    assert torch.allclose(EX.return_level_error(levels)[2], levels[0], rtol=1e-15, atol=0, equal_nan=True) and tuple(EX.regional_lmoments(lm, nv).shape) == (4, 2, 3)
    pit = EX.gev_pit(t.extremes, xi, alpha, k)
    fitted = ~torch.isnan(xi[0])
    assert tuple(pit.shape) == (3, 2, 10) and pit.sum(dim=-1).tolist() == [[8 * int(fitted[f].sum()) for f in range(2)]] * 3


def test_the_algebra_on_hand_made_maps():
    lm = torch.zeros((3, 1, 4, 1, 2), dtype=torch.float64)
    lm[0, 0, :, 0] = torch.tensor([[10.0, 20.0], [2.0, 4.0], [0.2, 0.4], [0.1, 0.4]], dtype=torch.float64)
    lm[1], lm[2] = lm[0] * 2, lm[0]
    lm[2, 0, 0] += torch.tensor([1.0, -3.0])
    bias, rmse = EX.mean_extreme_error(lm)
    assert bias.view(-1).tolist() == [15.0, -1.0] and rmse.view(-1).tolist() == [math.sqrt((100 + 400) / 2), math.sqrt((1 + 9) / 2)]
    t, t3, t4 = EX.lmoment_ratios(lm[0])
    assert t.view(-1).tolist() == [0.2, 0.2] and t3.view(-1).tolist() == [0.1, 0.1] and t4.view(-1).tolist() == [0.05, 0.1]
    reg = EX.regional_lmoments(lm[0], torch.tensor([[[1, 3]]], dtype=torch.int32))
    assert reg.view(-1).tolist() == pytest.approx([0.2, 0.1, (0.05 + 0.3) / 4], rel=1e-15)
    levels = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64).view(3, 1, 1, 1, 1).expand(3, 1, 2, 1, 2)
    b, r, mean = EX.return_level_error(levels)
    assert b.view(-1).tolist() == [1.0, 1.0, 3.0, 3.0] and r.view(-1).tolist() == [1.0, 1.0, 3.0, 3.0] and mean.view(-1).tolist() == [3.0] * 4


def test_the_report(route):
    _, _, xt, yt = _fields("smooth", 2, 48, 2, 2, 4, seed=6)
    samples = torch.cat([yt[None], xt])            # the truth as member 0
    rep = EX.extremes_report(samples, yt, 6, ["max", "min"], [2, 10], names=["gust", "pressure"])
    assert isinstance(rep, VariableReport) and rep.names == ["gust", "pressure"]
    v = rep["gust"]
    assert int(v["direction"]) == 1 and int(rep["pressure"]["direction"]) == 0 and v["n_blocks"] == 8 and v["periods"].tolist() == [2.0, 10.0]
    assert float(v["mean_extreme_bias"][0]) == 0.0 and float(v["return_level_bias"][0].abs().max()) == 0.0 and float(v["ratio_rmse"][0].abs().max()) == 0.0
    assert tuple(v["return_level_rmse"].shape) == (3, 2) and tuple(v["return_level_mean"].shape) == (2, 2, 4) and tuple(v["pit"].shape) == (3, 10)
    assert tuple(v["regional"].shape) == (4, 3) and tuple(v["unfitted"].shape) == (4,) and v["invalid"].tolist() == [0] * 4
    d = rep.as_dict()
    assert set(d) == {f"extremes/{n}/{k}{s}" for n in rep.names for k in ("mean_extreme_bias", "return_level_bias_p0", "return_level_bias_p1",
                                                                            "return_level_rmse_p0", "return_level_rmse_p1") for s in ("", "_std")}
    assert d["extremes/gust/mean_extreme_bias"] == pytest.approx(float(v["mean_extreme_bias"].mean()), rel=1e-15)
    assert rep.as_dict(prefix="x").keys() == {k.replace("extremes/", "x/", 1) for k in d}


def test_argument_errors_are_value_errors(route):
    _, _, xt, yt = _fields("smooth", 2, 6, 2, 2, 4)
    A = EX.ExtremeAccumulator
    for args, kw, text in (((0, 2, 2, 4, 3), dict(max_blocks=2), "M 0 must be an integer >= 1"), ((2, 2, 2, 4, 0), dict(max_blocks=2), "block 0 must be"),
                           ((2, 2, 2, 4, 3), dict(max_blocks=0), "max_blocks 0 must be"), ((2, 2, 2, 4, 2.5), dict(max_blocks=2), "block 2.5 must be"),
                           ((2, 2, 2, 4, 3, "up"), dict(max_blocks=2), "direction 'up' must be 'max' or 'min'"),
                           ((2, 2, 2, 4, 3, ["max"]), dict(max_blocks=2), "one of them per variable (2)")):
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)")):
            A(*args, **kw)
    with pytest.raises(TypeError):
        A(2, 2, 2, 4, 3)                                                  # max_blocks has no default
    acc = A(2, 2, 2, 4, 3, max_blocks=1)
    for call, text in ((lambda: acc.update(xt), "made with a truth"), (lambda: A(2, 2, 2, 4, 3, with_truth=False, max_blocks=1).update(xt, yt), "made without a truth"),
                       (lambda: acc.update(xt, yt[:5]), r"must be \(M >= 1,\) \+ truth"), (lambda: acc.update(xt.long(), yt.long()), "must be floating point"),
                       (lambda: acc.update(xt[:1], yt), r"must be \(M, T, F, H, W\) = \(2, T, 2, 2, 4\)"),
                       (lambda: A(2, 2, 2, 4, 3, with_truth=False, max_blocks=1).update(xt.long()), r"must be floating point \(M, T, F, H, W\)"),
                       (lambda: acc.update(xt, yt), "over max_blocks = 1"), (lambda: acc.tables("half"), "partial 'half' must be 'drop' or 'keep'"),
                       (lambda: EX.block_extremes(xt[0], yt, 3), r"must be \(M, T, F, H, W\)"), (lambda: EX.lmoments(torch.zeros(3, 4)), r"\(\.\.\., n >= 1, H, W\)"),
                       (lambda: EX.lmoment_ratios(torch.zeros(3, 2, 4)), r"lmom \(3, 2, 4\) must be \(\.\.\., 4, H, W\)"),
                       (lambda: EX.gev_return_level(torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 4), [1.0]), "at least one R > 1"),
                       (lambda: EX.gev_return_level(torch.zeros(2, 4), torch.zeros(2, 3), torch.zeros(2, 4), [2.0]), "must have one shape"),
                       (lambda: EX.mean_extreme_error(torch.zeros(1, 2, 4, 2, 4)), "row 0 the truth"),
                       (lambda: EX.lmoment_ratio_error(torch.zeros(2, 4, 2, 4)), r"must be \(D >= 2, F, 4, H, W\)"),
                       (lambda: EX.regional_lmoments(torch.zeros(2, 4, 2, 4), torch.zeros(2, 2, 3)), "lmom's without the moments"),
                       (lambda: EX.gev_pit(torch.zeros(2, 1, 3, 2, 4), torch.zeros(2, 1, 2, 3), torch.zeros(2, 1, 2, 3), torch.zeros(2, 1, 2, 3)), "and the fits"),
                       (lambda: EX.extremes_report(xt, yt, 3, "max", [2], names=["a"]), "1 names for 2 variables")):
        with pytest.raises(ValueError, match=text):
            call()
    sd = A(2, 2, 2, 4, 3, max_blocks=2).state_dict()
    for make, text in ((lambda: A(2, 2, 2, 4, 4, max_blocks=2), "block 3 of the state differs"), (lambda: A(2, 2, 2, 4, 3, "min", max_blocks=2), "directions of the state differ"),
                       (lambda: A(3, 2, 2, 4, 3, max_blocks=2), r"open \(3, 2, 8\) of the state must be \(4, 2, 8\)")):
        with pytest.raises(ValueError, match=text):
            make().load_state_dict(sd)


# ------------------------------------------------------------------------------------------------------------------ refusals

BAD_ARG, BAD_SHAPE, UNSUPPORTED = -1, -2, -3
DEV = object()   # a made-up device address: argument number i of a call is 4096 (16 + i); nothing dereferences it
M20 = 1 << 20
BASE = {
    "c2w_block_extremes_update": dict(x=DEV, y=DEV, dir=DEV, open=DEV, table=DEV, invalid=DEV, M=2, T=4, F=2, hw=16, block=2, max_blocks=8, t0=0, stream=None),
    "c2w_lmoments": dict(table=DEV, lmom=DEV, n_valid=DEV, R=4, n=8, hw=16, stream=None),
}
REFUSED = [
    ("c2w_block_extremes_update", [(f"{n} null", {n: None}, BAD_ARG) for n in ("x", "dir", "open", "table", "invalid")]
     + [(f"{n} off by 4", {n: 4}, BAD_ARG) for n in ("x", "y", "open", "table", "invalid")] + [("dir off by 2", dict(dir=2), BAD_ARG)]
     + [("hw = 6", dict(hw=6), UNSUPPORTED), ("block = 0", dict(block=0), UNSUPPORTED), ("block over 2^20", dict(block=M20 + 1), UNSUPPORTED),
        ("B over 4096", dict(max_blocks=4097), UNSUPPORTED), ("no member", dict(M=0), UNSUPPORTED), ("T over 2^20", dict(T=M20 + 1, block=M20), BAD_SHAPE),
        ("a block behind the table", dict(t0=16), BAD_SHAPE), ("grid", dict(M=M20, F=M20), BAD_SHAPE), ("t0 < 0", dict(t0=-1), BAD_ARG)]),
    ("c2w_lmoments", [(f"{n} null", {n: None}, BAD_ARG) for n in ("table", "lmom", "n_valid")]
     + [("table off by 4", dict(table=4), BAD_ARG), ("lmom off by 4", dict(lmom=4), BAD_ARG), ("n_valid off by 2", dict(n_valid=2), BAD_ARG),
        ("n = 65", dict(n=65), UNSUPPORTED), ("n = 0", dict(n=0), UNSUPPORTED), ("hw = 6", dict(hw=6), UNSUPPORTED), ("grid", dict(R=1 << 40), BAD_SHAPE)]),
]


def _arguments(name, change):
    """the base call of `name`, which would be valid and is never made, with `change` applied"""
    assert change and set(change) <= set(BASE[name])
    out = []
    for i, (arg, value) in enumerate(BASE[name].items()):
        address = 4096 * (16 + i)
        if arg in change:
            c = change[arg]
            value = address + c if value is DEV and isinstance(c, int) else c
        elif value is DEV:
            value = address
        out.append(value)
    return out


def test_the_refusal_rows_hold_no_valid_call():
    for name, cases in REFUSED:
        for what, change, code in cases:
            assert code < 0 and len(_arguments(name, change)) == len(_lib._PROTOS[name]), (name, what)


def test_the_launchers_refuse_out_of_range_geometry_before_any_launch():
    if torch.cuda.is_available():
        pytest.skip("made-up device addresses: only where nothing can launch")
    build.build(verbose=False)
    lib = _lib.load()
    wrong = [(name, what, rc, code) for name, cases in REFUSED for what, change, code in cases
             for rc in [getattr(lib, name)(*_arguments(name, change))] if rc != code]
    assert not wrong, wrong
    assert lib.c2w_block_extremes_supported(16, 24, 4096) == 1 and lib.c2w_block_extremes_supported(6, 24, 8) == 0
    assert lib.c2w_lmoments_supported(16, 64) == 1 and lib.c2w_lmoments_supported(16, 65) == 0


# ------------------------------------------------------------------------------------------------------------------ the host program

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_extremes(request, tmp_path_factory):
    """a stand-alone program, once plain and once under the address and undefined-behaviour sanitizers; it is run directly, never loaded
    into Python"""
    return host_program.build(tmp_path_factory, "extremes", sanitize=request.param == "sanitized", fp_contract_off=True, timeout=600)


@pytest.mark.parametrize("M,T,F,hw,block,B,has_truth,t0", [(1, 1, 1, 4, 1, 1, 0, 0), (2, 9, 2, 1028, 3, 8, 1, 4), (1, 8, 1, 2052, 24, 2, 1, 20),
                                                         (3, 7, 2, 1024, 2, 4, 0, 1), (1, 33, 1, 12, 5, 16, 1, 47), (1, 5, 1, 8, 9, 1, 1, 0)])
def test_every_cell_hour_is_read_once_and_every_closed_block_written_once(host_extremes, M, T, F, hw, block, B, has_truth, t0):
    """one thread, a chunk and a thread, three chunks, exactly one chunk; T around the unroll; a call that starts inside a block, one
    that ends a block with its last hour, one that ends none"""
    rc = subprocess.run([str(host_extremes), "visit"] + [str(a) for a in (M, T, F, hw, block, B, has_truth, t0)], timeout=600).returncode
    assert rc == 0, f"check {rc} of host_extremes_main.cpp failed"


@pytest.mark.parametrize("R_,n,hw", [(1, 1, 4), (2, 8, 1028), (1, 9, 1024), (3, 17, 2052), (1, 33, 516), (2, 64, 260)])
def test_every_block_extreme_is_read_once_by_the_moments(host_extremes, R_, n, hw):
    rc = subprocess.run([str(host_extremes), "lvisit", str(R_), str(n), str(hw)], timeout=600).returncode
    assert rc == 0, f"check {rc} of host_extremes_main.cpp failed"


def test_the_host_program_equals_the_reference_for_every_cut(host_extremes, tmp_path):
    """csrc/extremes_maps.h compiled for the host: every kind, every cut of T = 7 into calls held against the single call inside the
    program, and the single call against the loops over keys"""
    M, T, F, block = 2, 7, 2, 3
    for i, kind in enumerate(R.KINDS):
        hw, has_truth = (8, 1028)[i % 2] if kind in ("smooth", "nan_hours") else 8, i % 2
        x, y = R.field(kind, (M, T, F, hw), i, block), R.field(kind, (T, F, hw), i + 50, block)
        dirs = np.array([1, 0], np.int32)
        D, B = M + has_truth, 3
        files = [str(tmp_path / n) for n in ("x.f32", "y.f32", "dir.i32", "table.f32", "open.u32", "invalid.i64")]
        for a, p in zip((x, y, dirs), files):
            a.tofile(p)
        args = [str(a) for a in (M, T, F, hw, block, B, has_truth, -1 if hw == 8 else 0b001010)]
        rc = subprocess.run([str(host_extremes), "update"] + args + files, timeout=600).returncode
        assert rc == 0, (kind, rc)
        want, invalid = R.block_extremes(x, y if has_truth else None, block, [True, False])
        table = np.fromfile(files[3], np.uint32).reshape(D, F, B, hw)
        assert np.array_equal(table[:, :, :2], want) and np.all(table[:, :, 2] == 0x12345678), kind
        assert np.array_equal(np.fromfile(files[5], np.int64).reshape(D, F), invalid), kind
        keep, _ = R.block_extremes(x, y if has_truth else None, block, [True, False], True)
        op = torch.from_numpy(np.fromfile(files[4], np.uint32).view(np.int32).reshape(D, F, hw))
        assert np.array_equal(_bits(EX._values(EX._unsigned(op), EX._flip(torch.from_numpy(dirs)))), keep[:, :, 2]), kind


@pytest.mark.parametrize("n", NS)
def test_the_host_programs_moments_lie_within_the_bound_and_equal_the_emulation(host_extremes, tmp_path, n):
    hw, Rr = 8, 3
    t = np.concatenate([_table("pressure", 1, n, hw, n), _table("smooth", 1, n, hw, n + 1, nan_share=0.3), _table("denormal", 1, n, hw, n + 2)])
    files = [str(tmp_path / f) for f in ("table.f32", "lmom.f64", "nvalid.i32")]
    t.tofile(files[0])
    assert subprocess.run([str(host_extremes), "lmoments", str(Rr), str(n), str(hw)] + files, timeout=600).returncode == 0
    lm, nv = np.fromfile(files[1], np.float64).reshape(Rr, 4, hw), np.fromfile(files[2], np.int32).reshape(Rr, hw)
    worst = R.check_lmoments(t, lm, nv)
    print(f"n = {n}: worst fraction of the bound {worst:.3f}")
    emu_lm, emu_nv = torch.empty((Rr, 4, hw), dtype=torch.float64), torch.empty((Rr, hw), dtype=torch.int32)
    assert emu_extreme_ops.lmoments(torch.from_numpy(t), emu_lm, emu_nv, Rr, n, hw)
    assert np.array_equal(emu_lm.numpy(), lm, equal_nan=True) and np.array_equal(emu_nv.numpy(), nv)   # the NumPy restatement: the same bits


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_block_extremes_supported": "int", "c2w_block_extremes_update": "int", "c2w_lmoments_supported": "int", "c2w_lmoments": "int"}
    c_abi.assert_declared(names, "extremes.hip", extreme_ops, ("update_supported", "lmoments_supported", "block_extremes_update", "lmoments"))
