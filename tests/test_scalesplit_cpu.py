"""The scale split of an ensemble without a GPU (climate2weather_amd/scalesplit.py, csrc/blockmoments_maps.h): the block-moment tables of
both routes -- the float64 torch definition and the emulation of the launcher standing in for the library -- against the NumPy
reference, bit for bit, for every field kind and block size; the sums against rational arithmetic within the bound
blockmoments_maps.h derives, and the fp32 avg_pool2d route's miss of it; the identity of the split in rational arithmetic; known
answers on integer fields; what the module and the launcher refuse; and the header compiled for the host as a program of its own, plain
and under the sanitizers."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import c_abi
import emu_blockmoment_ops
import fp64_blockmoments_ref as R
import host_program
from climate2weather_amd import _lib, build, scale_ops
from climate2weather_amd import scalesplit as SS
from climate2weather_amd.ensemble_host import VariableReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 4, 8, 16, 32)


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of scalesplit.py on CPU tensors"""
    if request.param == "launcher":
        emu_blockmoment_ops.install(monkeypatch, scale_ops, SS)
    return request.param


def _fields(kind, M, T, F, H, W, seed=0):
    x, y = R.field(kind, (M, T, F, H, W), seed), R.field(kind, (T, F, H, W), seed + 1)
    return x, y, torch.from_numpy(x), torch.from_numpy(y)


def _same(st, t):
    return R.same_bits(st, t.n.numpy(), t.pivot.numpy(), t.sums.numpy())


def _integers(shape, seed, low=-20, high=20):
    return np.random.default_rng(seed).integers(low, high, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the tables

@pytest.mark.parametrize("kind", R.KINDS)
def test_the_tables_equal_the_reference_bit_for_bit(route, kind):
    """general route = reference = emulation, as bits: every block size, with and without a truth; 2 x 3 blocks a plane"""
    M, T, F = 2, 2, 2
    for s in SIZES:
        H, W = 2 * s, 3 * s
        x, y, xt, yt = _fields(kind, M, T, F, H, W, seed=s)
        for with_truth in (True, False):
            t = SS.block_moments(xt, yt if with_truth else None, s)
            D, NS = M + with_truth, 3 if with_truth else 2
            assert t.s == s and t.with_truth == with_truth and tuple(t.sums.shape) == (D, T, F, NS, 2, 3) and t.sums.dtype == torch.float64
            assert tuple(t.n.shape) == (D, T, F, 2, 3) and t.n.dtype == torch.int32 and tuple(t.pivot.shape) == (D, T, F, 2, 3) and t.pivot.dtype == torch.float32
            assert _same(R.block_moments(x, y if with_truth else None, s), t), (kind, s, with_truth)
    if route == "launcher":
        assert len(emu_blockmoment_ops.CALLS) == 8 and emu_blockmoment_ops.CALLS[0] == (M, T, F, 8, 12, 4, True)   # s = 2 asked "supported" only


def test_a_ragged_last_workgroup_and_exactly_one_workgroup_a_plane(route):
    """258 items at s = 4; 256 items a plane at s = 16"""
    for s, H, W in ((4, 8, 516), (16, 128, 128)):
        x, y, xt, yt = _fields("nan_cells", 1, 1, 2, H, W, seed=s)
        assert _same(R.block_moments(x, y, s), SS.block_moments(xt, yt, s)), s


def test_row_zero_carries_the_truth_against_itself(route):
    x, y, xt, yt = _fields("nan_cells", 2, 2, 1, 16, 16, seed=5)
    t = SS.block_moments(xt, yt, 4)
    assert torch.equal(t.sums[0, :, :, 2].view(torch.int64), t.sums[0, :, :, 1].view(torch.int64))
    alone = SS.block_moments(yt[None], None, 4)
    assert torch.equal(alone.sums[0].view(torch.int64), t.sums[0, :, :, :2].view(torch.int64)) and torch.equal(alone.n[0], t.n[0])


def test_an_invalid_block_is_canonical_nan_and_counted_and_its_neighbours_are_unaffected(route):
    s, M, T, F, H, W = 4, 2, 1, 1, 12, 12
    x, y, xt, yt = _fields("smooth", M, T, F, H, W, seed=7)
    clean = SS.block_moments(xt, yt, s)
    xb, yb = xt.clone(), yt.clone()
    xb[0, 0, 0, 5, 6] = float("nan")      # member 0, block (1, 1)
    xb[1, 0, 0, 0, 0] = float("inf")      # member 1, block (0, 0): its pivot
    yb[0, 0, 9, 2] = float("-inf")        # the truth, block (2, 0)
    t = SS.block_moments(xb, yb, s)
    bits = t.sums.view(torch.int64)
    nan = 0x7FF8000000000000
    assert t.n[1, 0, 0, 1, 1] == 15 and t.n[2, 0, 0, 0, 0] == 15 and t.n[0, 0, 0, 2, 0] == 15 and int((t.n != 16).sum()) == 3
    assert bits[1, 0, 0, :, 1, 1].tolist() == [nan] * 3 and bits[2, 0, 0, :, 0, 0].tolist() == [nan] * 3 and bits[0, 0, 0, :, 2, 0].tolist() == [nan] * 3
    assert bits[1:, 0, 0, 2, 2, 0].tolist() == [nan] * 2                          # X of the members where the truth's block is invalid
    assert not bool(torch.isnan(t.sums[1:, 0, 0, :2, 2, 0]).any())                # their own sums there are numbers
    assert int(torch.isnan(t.sums).sum()) == 3 + 3 + 3 + 2
    same = ~torch.isnan(t.sums)
    assert torch.equal(t.sums[same].view(torch.int64), clean.sums[same].view(torch.int64))
    assert torch.isinf(t.pivot[2, 0, 0, 0, 0])
    split, ratio = SS.error_split(t), SS.variance_ratio(t)
    assert split.invalid[:, 0, 0].tolist() == [2, 2] and split.blocks[:, 0, 0].tolist() == [7, 7] and ratio.invalid[:, 0, 0].tolist() == [2, 2]
    assert bool(torch.isfinite(split.total).all()) and bool(torch.isfinite(ratio.per_time).all()) and bool(torch.isfinite(SS.detail_correlation(t).pooled).all())
    keep = torch.ones(3, 3, dtype=torch.bool)
    keep[1, 1] = keep[2, 0] = False       # member 0's valid blocks, by hand from the clean tables
    p = SS._parts(clean)
    want = (16.0 * p.dm[0, 0, 0] ** 2)[keep].sum() / (16.0 * 7)
    assert float(split.coarse[0, 0, 0]) == pytest.approx(float(want), rel=1e-14)


def test_strided_and_half_precision_inputs(route):
    x, y, xt, yt = _fields("smooth", 2, 2, 2, 8, 8)
    big = torch.zeros((2, 2, 2, 8, 16))
    big[..., ::2] = xt
    a, b = SS.block_moments(big[..., ::2], yt, 4), SS.block_moments(xt, yt, 4)
    assert torch.equal(a.sums, b.sums) and torch.equal(a.pivot, b.pivot)
    h = SS.block_moments(xt.half(), yt.double(), 4)
    assert torch.equal(h.sums, SS.block_moments(xt.half().float(), yt, 4).sums)
    off = torch.zeros(2 * 2 * 2 * 8 * 8 + 1)[1:].view(2, 2, 2, 8, 8).copy_(xt)   # dense fp32, 4 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 != 0 and torch.equal(SS.block_moments(off, yt, 4).sums, b.sums)


def test_an_unsupported_shape_reaches_only_supported(monkeypatch):
    emu_blockmoment_ops.install(monkeypatch, scale_ops, SS)
    assert not scale_ops.supported(8, 8, 2) and not scale_ops.supported(8, 20, 8) and not scale_ops.supported(64, 64, 64) and scale_ops.supported(8, 24, 8)
    for s, H, W in ((2, 4, 6), (5, 10, 5), (64, 64, 64)):
        x, y, xt, yt = _fields("nan_cells", 1, 2, 1, H, W)
        assert _same(R.block_moments(x, y, s), SS.block_moments(xt, yt, s))
    assert emu_blockmoment_ops.CALLS == []   # the launcher was asked "supported" only


def test_the_emulation_restates_the_constants_of_the_kernel():
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "blockmoments_maps.h")).read()
    for text in ("THREADS = 256", "GROUP = 8", "CANONICAL_NAN = 0x7ff8000000000000ull", "return s == 4 || s == 8 || s == 16 || s == 32;",
                 "return truth ? 3 : 2;", "size_ok(s) && H >= s && W >= s && H % s == 0 && W % s == 0", "return (long long)(H / s) * (W / 4);",
                 "return (items + THREADS - 1) / THREADS;", "& 0x7F800000u) != 0x7F800000u", "return 2 * s + (product ? 2 : 0);", "clang fp contract(off)"):
        assert text in core, text
    e = emu_blockmoment_ops
    assert (e.THREADS, e.GROUP, e.SIZES) == (256, 8, (4, 8, 16, 32)) and SS.DEVICE_SIZES == e.SIZES and int(e.NAN_BITS) == SS._NAN == int(R.NAN_BITS)
    assert all(e.bound_rounds(s, p) == R.bound_rounds(s, p) == 2 * s + 2 * p for s in SIZES for p in (False, True))
    assert e.row_items(3, 8, 516, 4) == 3 * 258 and e.chunks(258) == 2 and e.entries(True) == 3 and e.entries(False) == 2
    assert '#include "core_side.h"' in core and not any(f"#define C2W_{side}" in core for side in ("HD", "BOTH", "CORE_HOST"))


# ------------------------------------------------------------------------------------------------------------------ the bound

@pytest.mark.parametrize("s", SIZES)
def test_the_sums_lie_within_the_derived_bound(route, s):
    """against ``fractions.Fraction`` on chosen blocks: the corners and a draw"""
    worst = 0.0
    for kind in ("pressure", "pressure_tight", "smooth", "denormal", "huge", "neg_zero", "nan_cells"):
        M, T, F, H, W = 1, 2, 1, 2 * s, 2 * s
        x, y, xt, yt = _fields(kind, M, T, F, H, W, seed=s)
        t = SS.block_moments(xt, yt, s)
        st = dict(n=t.n.numpy(), pivot=t.pivot.numpy(), sums=t.sums.numpy(), s=s)
        worst = max(worst, R.check_bound(x, y, st, R.chosen_blocks(st["n"].shape, 6 if s < 32 else 3, seed=s)))
    print(f"s = {s} ({route}): worst fraction of the bound {worst:.4f}")


def test_the_fp32_avg_pool_route_misses_the_bound_on_pressure_at_32():
    """``avg_pool2d`` in fp32 -- the route a user would write -- as ``S1 = N (mean - pivot)``, against the exact ``S1`` and the bound the
    pivoted sums are held to.  ``pressure`` is 101325 +- 0.5: the fp32 mean is wrong in its last bits, units of 2^-7, and the bound
    is of order 2 s 2^-53 N / 2."""
    s, N = 32, 32 * 32
    x, _, xt, _ = _fields("pressure", 1, 1, 1, 2 * s, 2 * s, seed=1)
    t = SS.block_moments(xt, None, s)
    pooled = torch.nn.functional.avg_pool2d(xt[0], s)                           # (1, 1, 2, 2) fp32
    factors = []
    for i in range(2):
        for j in range(2):
            exact, absolute = R.exact_block(x[0, 0, 0, i * s:(i + 1) * s, j * s:(j + 1) * s], None)
            limit = R.bound_rounds(s, False) * R.U * absolute[0]
            mine = abs(Fraction(float(t.sums[0, 0, 0, 0, i, j])) - exact[0])
            theirs = abs((Fraction(float(pooled[0, 0, i, j])) - Fraction(float(t.pivot[0, 0, 0, i, j]))) * N - exact[0])
            assert mine <= limit
            factors.append(float(theirs / limit))
    print(f"fp32 avg_pool2d error of S1 over the bound at s = 32: {min(factors):.3g} .. {max(factors):.3g}")
    assert max(factors) > 1e6   # eight digits between fp32 and the bound's 2^-47 relative; two of them for a lucky block


# ------------------------------------------------------------------------------------------------------------------ the identity

@pytest.mark.parametrize("kind", ["pressure", "smooth"])
def test_the_split_adds_up_to_the_mean_squared_error_in_rational_arithmetic(route, kind):
    M, T, F, H, W = 2, 2, 1, 16, 16
    x, y, xt, yt = _fields(kind, M, T, F, H, W, seed=11)
    for s in (2, 4, 16):
        split = SS.error_split(SS.block_moments(xt, yt, s))
        for m in range(M):
            for t in range(T):
                exact = R.exact_mse(x[m, t, 0], y[t, 0])
                rel = abs(Fraction(float(split.total[m, t, 0])) - exact) / exact
                print(f"{kind} s = {s} ({route}): total against the exact mean square, relative {float(rel):.3g}")
                assert rel <= Fraction(1, 10 ** 12), (kind, s, m, t, float(rel))
                assert float(split.total[m, t, 0]) == float(split.coarse[m, t, 0]) + float(split.detail[m, t, 0])


# ------------------------------------------------------------------------------------------------------------------ known answers

def test_members_equal_to_the_truth(route):
    y = _integers((3, 2, 16, 16), 1)
    yt = torch.from_numpy(y)
    for s in (2, 4, 8):
        t = SS.block_moments(yt[None].expand(2, -1, -1, -1, -1), yt, s)
        split, ratio, corr = SS.error_split(t), SS.variance_ratio(t), SS.detail_correlation(t)
        assert float(split.coarse.abs().max()) == 0.0 and float(split.detail.abs().max()) == 0.0 and float(split.total.abs().max()) == 0.0
        assert ratio.per_time.unique().tolist() == [1.0] and ratio.pooled.unique().tolist() == [1.0]
        assert corr.per_time.unique().tolist() == [1.0] and corr.pooled.unique().tolist() == [1.0]
        assert bool(torch.isnan(split.coarse_share).all()) and int(split.invalid.sum()) == 0


def test_a_member_that_is_the_truth_plus_a_constant_per_block(route):
    s, H, W = 4, 16, 12
    y = _integers((2, 2, H, W), 2)
    k = _integers((2, 2, H // s, W // s), 3, -5, 6)
    x = (y + np.repeat(np.repeat(k, s, axis=-2), s, axis=-1))[None]
    t = SS.block_moments(torch.from_numpy(x), torch.from_numpy(y), s)
    split = SS.error_split(t)
    assert float(split.detail.abs().max()) == 0.0
    assert torch.equal(split.coarse[0], torch.from_numpy((k.astype(np.float64) ** 2).mean(axis=(-1, -2))))
    assert split.coarse_share[split.coarse > 0].unique().tolist() == [1.0]
    assert SS.variance_ratio(t).per_time.unique().tolist() == [1.0] and SS.detail_correlation(t).per_time.unique().tolist() == [1.0]
    assert torch.equal(SS.coarse(t)[1] - SS.coarse(t)[0], torch.from_numpy(k.astype(np.float64)))


def test_a_member_constant_on_every_block(route):
    s, H, W = 4, 8, 8
    y = _integers((2, 1, H, W), 4)
    k = _integers((2, 1, H // s, W // s), 5)
    x = np.repeat(np.repeat(k, s, axis=-2), s, axis=-1)[None]
    t = SS.block_moments(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(y), s)
    split = SS.error_split(t)
    assert float(SS.variance_ratio(t).per_time.abs().max()) == 0.0 and float(SS.variance_ratio(t).pooled.abs().max()) == 0.0
    assert torch.equal(split.detail[0], SS.subgrid_variance(t)[0].mean(dim=(-1, -2)))
    assert float(SS.subgrid_variance(t)[1].abs().max()) == 0.0 and bool(torch.isnan(SS.detail_correlation(t).per_time).all())
    yb = R.blocks(y.astype(np.float64), s)
    assert np.array_equal(SS.subgrid_variance(t)[0].numpy(), yb.var(axis=(-1, -2))) and np.array_equal(SS.coarse(t)[0].numpy(), yb.mean(axis=(-1, -2)))


def test_the_truth_row_reproduces_its_own_observation(route):
    s, t_step = 4, 3
    y = _integers((7, 2, 8, 8), 6)
    x = _integers((2, 7, 2, 8, 8), 7)
    t = SS.block_moments(torch.from_numpy(x), torch.from_numpy(y), s)
    obs = SS.coarse(t)[0, ::t_step]
    assert tuple(obs.shape) == (3, 2, 2, 2)
    res = SS.observation_residual(t, obs, t_step)
    assert tuple(res.bias.shape) == (3, 3, 2) and res.blocks.unique().tolist() == [4]
    assert float(res.bias[0].abs().max()) == 0.0 and float(res.rmse[0].abs().max()) == 0.0 and float(res.max_abs[0].abs().max()) == 0.0
    assert float(res.rmse[1:].min()) > 0.0
    pooled = torch.nn.functional.avg_pool2d(torch.from_numpy(x).double()[:, ::t_step].reshape(-1, 2, 8, 8), s).view(2, 3, 2, 2, 2)
    assert torch.equal(res.max_abs[1:], (pooled - obs).abs().amax(dim=(-1, -2)))   # integers: avg_pool2d in float64 is exact too
    assert torch.equal(res.bias[1:], (pooled - obs).mean(dim=(-1, -2)))


def test_the_scores_agree_with_numpy_on_a_smooth_field(route):
    M, T, F, H, W, s = 2, 3, 2, 16, 24, 8
    x, y, xt, yt = _fields("smooth", M, T, F, H, W, seed=21)
    t = SS.block_moments(xt, yt, s)
    xb, yb = R.blocks(x.astype(np.float64), s), R.blocks(y.astype(np.float64), s)
    mx, my = xb.mean(axis=(-1, -2), keepdims=True), yb.mean(axis=(-1, -2), keepdims=True)
    assert np.allclose(SS.coarse(t).numpy()[1:], mx[..., 0, 0], rtol=1e-13) and np.allclose(SS.subgrid_variance(t).numpy()[0], yb.var(axis=(-1, -2)), rtol=1e-11)
    dx, dy = xb - mx, (yb - my)[None]
    split, ratio, corr = SS.error_split(t), SS.variance_ratio(t), SS.detail_correlation(t)
    assert np.allclose(split.coarse.numpy(), ((mx - my[None]) ** 2).mean(axis=(-1, -2, -3, -4)), rtol=1e-11)
    assert np.allclose(split.detail.numpy(), ((dx - dy) ** 2).mean(axis=(-1, -2, -3, -4)), rtol=1e-11)
    assert np.allclose(split.total.numpy(), ((x.astype(np.float64) - y.astype(np.float64)[None]) ** 2).mean(axis=(-1, -2)), rtol=1e-11)
    assert np.allclose(ratio.per_time.numpy(), (dx ** 2).sum(axis=(-1, -2, -3, -4)) / (dy ** 2).sum(axis=(-1, -2, -3, -4)), rtol=1e-11)
    assert np.allclose(ratio.pooled.numpy(), (dx ** 2).sum(axis=(1, -1, -2, -3, -4)) / (dy ** 2).sum(axis=(1, -1, -2, -3, -4)), rtol=1e-11)
    want = (dx * dy).sum(axis=(-1, -2, -3, -4)) / np.sqrt((dx ** 2).sum(axis=(-1, -2, -3, -4)) * (dy ** 2).sum(axis=(-1, -2, -3, -4)))
    assert np.allclose(corr.per_time.numpy(), want, rtol=1e-10, atol=1e-12)
    assert np.allclose(split.coarse_share.numpy(), split.coarse.numpy() / split.total.numpy(), rtol=1e-15)


def test_the_scale_profile_moves_the_error_from_detail_to_coarse(route):
    M, T, F, H, W = 2, 2, 2, 32, 32
    x, y, xt, yt = _fields("smooth", M, T, F, H, W, seed=31)
    prof = SS.scale_profile(xt, yt)
    assert prof.scales == (2, 4, 8, 16, 32)
    for a in (prof.coarse, prof.detail, prof.variance_ratio, prof.detail_correlation):
        assert tuple(a.shape) == (5, M, F) and a.dtype == torch.float64
    total = ((x.astype(np.float64) - y.astype(np.float64)[None]) ** 2).mean(axis=(1, 3, 4))
    assert np.allclose((prof.coarse + prof.detail).numpy(), total[None], rtol=1e-11)           # the same error at every scale
    assert bool((prof.detail[1:] >= prof.detail[:-1]).all()) and bool((prof.coarse[1:] <= prof.coarse[:-1]).all())   # nested blocks
    one = SS.error_split(SS.block_moments(xt[:, :1], yt[:1], 8))
    assert np.allclose(SS.scale_profile(xt[:, :1], yt[:1], scales=(8,)).detail[0].numpy(), one.detail[:, 0].numpy(), rtol=1e-14)
    if route == "launcher":
        assert [c[5] for c in emu_blockmoment_ops.CALLS][:4] == [4, 8, 16, 32]


def test_the_reports_keys_and_shapes(route):
    M, L, F, H, W, s, t_step = 3, 7, 2, 16, 16, 4, 6
    x, y, xt, yt = _fields("nan_cells", M, L, F, H, W, seed=14)
    obs = torch.nn.functional.avg_pool2d(torch.nan_to_num(yt)[::t_step], s)
    rep = SS.scales_report(xt, yt, observation=obs, names=["u", "p"])
    assert isinstance(rep, VariableReport) and rep.names == ["u", "p"] and rep.s == 4 and rep.t_step == 6
    per_member = ("coarse", "detail", "total", "coarse_share", "variance_ratio", "detail_correlation", "observation_bias", "observation_rmse", "observation_max_abs")
    shapes = {k: (M,) for k in per_member}
    shapes.update({f"{k}_per_time": (M, L) for k in per_member[:6]}, invalid_blocks=(M,), truth_observation_rmse=())
    for name, v in rep:
        assert set(v) == set(shapes)
        for key, shape in shapes.items():
            assert tuple(v[key].shape) == shape, (name, key)
            assert v[key].dtype == (torch.int64 if key == "invalid_blocks" else torch.float64), key
        assert int(v["invalid_blocks"].min()) > 0
    flat = rep.as_dict()
    assert set(flat) == {f"scales/{n}/{k}{e}" for n in rep.names for k in per_member for e in ("", "_std")} and all(isinstance(v, float) for v in flat.values())
    assert flat["scales/u/coarse"] == pytest.approx(float(rep["u"]["coarse"].mean()))
    plain = SS.scales_report(xt, yt)
    assert plain.s == 16 and plain.t_step is None and "observation_rmse" not in plain["var0"] and set(plain.as_dict()) == {
        f"scales/{n}/{k}{e}" for n in ("var0", "var1") for k in per_member[:6] for e in ("", "_std")}
    every = SS.scales_report(xt, yt, observation=torch.zeros(L, F, 2, 2))
    assert every.s == 8 and every.t_step == 1
    assert SS.ScalesReport([], [], 16, None).as_dict() == {}


# ------------------------------------------------------------------------------------------------------------------ refusals of the module

def test_what_the_module_refuses():
    x, y, xt, yt = _fields("smooth", 2, 6, 2, 8, 8)
    t = SS.block_moments(xt, yt, 4)
    alone = SS.block_moments(xt, None, 4)
    for call, text in ((lambda: SS.block_moments(xt, yt[:5], 4), r"must be \(M >= 1,\) \+ truth"), (lambda: SS.block_moments(xt.long(), yt.long(), 4), "must be floating point"),
                       (lambda: SS.block_moments(xt[0], None, 4), r"must be floating point \(M >= 1, T, F, H, W\)"),
                       (lambda: SS.block_moments(xt, yt, 3), "s = 3 must divide H = 8 and W = 8"), (lambda: SS.block_moments(xt, yt, 0), "s 0 must be an integer >= 1"),
                       (lambda: SS.block_moments(xt, yt, 2.5), "s 2.5 must be an integer >= 1"), (lambda: SS.block_moments(xt, yt, 16), "s = 16 must divide"),
                       (lambda: SS.error_split(alone), "error_split needs tables with a truth"), (lambda: SS.variance_ratio(alone), "needs tables with a truth"),
                       (lambda: SS.detail_correlation(alone), "needs tables with a truth"),
                       (lambda: SS.observation_residual(t, torch.zeros(2, 2, 2, 2), 6), r"must be \(ceil\(T / t_step\), F, h, w\) = \(1, 2, 2, 2\)"),
                       (lambda: SS.observation_residual(t, torch.zeros(1, 2, 2, 2), 0), "t_step 0 must be an integer >= 1"),
                       (lambda: SS.scale_profile(xt, yt, scales=(4, 16)), "s = 16 must divide"),
                       (lambda: SS.scales_report(xt, yt, observation=torch.zeros(1, 2, 3, 3)), "with h a divisor of H = 8"),
                       (lambda: SS.scales_report(xt, yt, names=["a"]), "1 names for 2 variables")):
        with pytest.raises(ValueError, match=text):
            call()
    assert tuple(SS.coarse(alone).shape) == (2, 6, 2, 2, 2) and tuple(SS.subgrid_variance(alone).shape) == (2, 6, 2, 2, 2)   # no truth needed


# ------------------------------------------------------------------------------------------------------------------ refusals of the launcher

BAD_ARG, BAD_SHAPE, UNSUPPORTED = -1, -2, -3
DEV = object()   # a made-up device address: argument number i of a call is 4096 (16 + i); nothing dereferences it
BASE = dict(x=DEV, y=DEV, n=DEV, pivot=DEV, sums=DEV, M=2, T=4, F=2, H=16, W=16, s=4, stream=None)
REFUSED = ([(f"{n} null", {n: None}, BAD_ARG) for n in ("x", "n", "pivot", "sums")]
           + [(f"{n} off by 4", {n: 4}, BAD_ARG) for n in ("x", "y", "sums")] + [(f"{n} off by 2", {n: 2}, BAD_ARG) for n in ("n", "pivot")]
           + [("s = 2", dict(s=2), UNSUPPORTED), ("s = 64", dict(s=64, H=64, W=64), UNSUPPORTED), ("W = 20, s = 8", dict(W=20, s=8), UNSUPPORTED),
              ("H = 20, s = 8", dict(H=20, s=8), UNSUPPORTED), ("H = 0", dict(H=0), UNSUPPORTED), ("no member", dict(M=0), UNSUPPORTED),
              ("F = 0", dict(F=0), UNSUPPORTED), ("T < 0", dict(T=-1), UNSUPPORTED), ("items beyond an int", dict(T=1 << 20, F=1 << 8, H=128, W=128), UNSUPPORTED),
              ("grid", dict(M=0x7FFFFFFE, T=1 << 10, H=128, W=128), UNSUPPORTED)])


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
    assert all(code < 0 and len(_arguments(change)) == len(_lib._PROTOS["c2w_block_moments"]) for _, change, code in REFUSED)
    if torch.cuda.is_available():
        pytest.skip("made-up device addresses: only where nothing can launch")
    build.build(verbose=False)
    lib = _lib.load()
    wrong = [(what, rc, code) for what, change, code in REFUSED for rc in [lib.c2w_block_moments(*_arguments(change))] if rc != code]
    assert not wrong, wrong
    assert lib.c2w_block_moments(*_arguments(dict(T=0))) == 0   # T = 0 returns 0 and writes nothing
    assert lib.c2w_block_moments_supported(64, 96, 32) == 1 and lib.c2w_block_moments_supported(8, 8, 2) == 0 and lib.c2w_block_moments_supported(16, 20, 8) == 0


# ------------------------------------------------------------------------------------------------------------------ the host program

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_blockmoments(request, tmp_path_factory):
    """a stand-alone program, once plain and once under the address and undefined-behaviour sanitizers; it is run directly, never loaded
    into Python"""
    return host_program.build(tmp_path_factory, "blockmoments", sanitize=request.param == "sanitized", fp_contract_off=True, timeout=900)


SHAPES = [(4, 4, 4), (4, 8, 516), (8, 8, 8), (8, 16, 24), (16, 16, 16), (16, 128, 128), (32, 32, 32), (32, 64, 96)]


@pytest.mark.parametrize("s,H,W", SHAPES)
def test_every_cell_is_read_once_and_every_block_stored_once(host_blockmoments, s, H, W):
    """one item, a ragged second workgroup, several blocks, exactly one workgroup a plane; three rows of two planes"""
    for has_truth in (0, 1):
        rc = subprocess.run([str(host_blockmoments), "visit"] + [str(a) for a in (2, 2, 1, H, W, s, has_truth)], timeout=600).returncode
        assert rc == 0, f"check {rc} of host_blockmoments_main.cpp failed"


@pytest.mark.parametrize("s,H,W", SHAPES)
def test_the_host_program_equals_the_reference_and_the_emulation(host_blockmoments, tmp_path, s, H, W):
    """csrc/blockmoments_maps.h compiled for the host: every kind in turn; the program's own straight-line restatement, the NumPy
    reference and the emulation of the launcher all give the same bits"""
    M, T, F = 2, 1, 2
    for i, kind in enumerate(R.KINDS):
        if H * W > 4096 and i % 3:
            continue                                      # the large planes take every third kind
        has_truth = (i + s // 4) % 2
        x, y = R.field(kind, (M, T, F, H, W), i), R.field(kind, (T, F, H, W), i + 50)
        files = [str(tmp_path / n) for n in ("x.f32", "y.f32", "n.i32", "pivot.f32", "sums.f64")]
        x.tofile(files[0]), y.tofile(files[1])
        rc = subprocess.run([str(host_blockmoments), "run"] + [str(a) for a in (M, T, F, H, W, s, has_truth)] + files, timeout=600).returncode
        assert rc == 0, (kind, rc)
        D, NS, h, w = M + has_truth, 2 + has_truth, H // s, W // s
        got = [np.fromfile(p, dt).reshape(shape) for p, dt, shape in zip(files[2:], (np.int32, np.float32, np.float64),
                                                                         ((D, T, F, h, w), (D, T, F, h, w), (D, T, F, NS, h, w)))]
        assert R.same_bits(R.block_moments(x, y if has_truth else None, s), *got), kind
        n, pivot = torch.zeros((D, T, F, h, w), dtype=torch.int32), torch.zeros((D, T, F, h, w))
        sums = torch.zeros((D, T, F, NS, h, w), dtype=torch.float64)
        assert emu_blockmoment_ops.block_moments(torch.from_numpy(x), torch.from_numpy(y) if has_truth else None, n, pivot, sums, M, T, F, H, W, s)
        assert R.same_bits(dict(n=got[0], pivot=got[1], sums=got[2]), n.numpy(), pivot.numpy(), sums.numpy()), kind


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_block_moments_supported": "int", "c2w_block_moments": "int"}
    c_abi.assert_declared(names, "blockmoments.hip", scale_ops, ("supported", "block_moments"))
