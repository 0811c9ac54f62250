"""CPU checks of the energy score and the variogram score (climate2weather_amd.multivariate): the energy score at d = 1 against
``crps.crps`` and the exactly integrated CRPS, the algebra of the fair and the joint forms, what the variogram score sees and the CRPS
does not, both routes of every public function -- the general float64 one and the launcher's, with tests/emu_escore_ops.py standing in
for the HIP kernels -- against the float64 definitions by the rules of tests/fp64_escore_ref.py, the D2 rule's negative control (the
fp32 Gram form fails it), the report, the argument checks, the kernels' own index maps and arithmetic compiled for the host
(csrc/escore_core.h) under the address and undefined-behaviour sanitizers, and the C declarations against the ctypes prototypes."""
import os
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_escore_ops
import fp64_crps_ref as CR
import fp64_escore_ref as R
import host_program
from climate2weather_amd import crps as C
from climate2weather_amd import escore_ops
from climate2weather_amd import multivariate as MV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of multivariate.pair_sqdist and variogram_terms on CPU tensors"""
    if request.param == "launcher":
        emu_escore_ops.install(monkeypatch, escore_ops, MV)
    return request.param


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))


def _t5(x, y, H, W_):
    """(M, T, F, hw), (T, F, hw) arrays -> the (M, T, F, H, W), (T, F, H, W) tensors of the public interface"""
    return torch.tensor(x).view(x.shape[:3] + (H, W_)), torch.tensor(y).view(y.shape[:2] + (H, W_))


def _smooth(M, T, F, H, W_, seed=0, noise=0.05):
    """members and truth that share a smooth field per plane, each with a smooth departure of its own (a draw of one coefficient) and a
    little noise, on a grid of 1 / 64 (sums with an integer stay exact in fp32)"""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W_), indexing="ij")
    base = 3.0 * np.sin(0.4 * ii + 0.3)[None, None] * np.cos(0.3 * jj)[None, None] * (1.0 + 0.5 * np.arange(F))[None, :, None, None]
    base = base + rng.standard_normal((T, 1, 1, 1))
    own = np.cos(0.5 * ii + 0.2 * jj)[None, None]
    x = base[None] + rng.standard_normal((M, T, F, 1, 1)) * own[None] + noise * rng.standard_normal((M, T, F, H, W_))
    y = base + rng.standard_normal((T, F, 1, 1)) * own + noise * rng.standard_normal((T, F, H, W_))
    q = lambda a: torch.tensor(np.round(a * 64.0) / 64.0, dtype=torch.float32)
    return q(x), q(y)


# ------------------------------------------------------------------------------------------------------------------ the definitions

@pytest.mark.parametrize("M", [1, 2, 5, 8])
def test_the_energy_score_at_d_1_is_the_crps(route, M):
    """one cell a plane (H = W = 1), beta = 1: against crps.crps (its general route) and against the integral
    (F_M(z) - 1[z >= y])^2 dz evaluated exactly in float64, to 1e-12"""
    rng = np.random.default_rng(M)
    T, F = 40, 3
    x = (rng.standard_normal((M, T, F, 1, 1)) * rng.uniform(0.1, 3.0, (1, T, F, 1, 1)) + rng.uniform(-5, 5, (1, T, F, 1, 1))).astype(np.float32)
    y = (2.0 * rng.standard_normal((T, F, 1, 1))).astype(np.float32)
    x[:, 0], y[0] = np.round(x[:, 0]), np.round(y[0])  # ties among the members and with the truth
    x[:, 1] = 2.5
    S, Tr = torch.tensor(x), torch.tensor(y)
    es = MV.energy_score(S, Tr).numpy()
    assert es.shape == (T, F) and es.dtype == np.float64
    want = C.crps(S, Tr).numpy()
    exact = np.array([[CR.crps_integral(x[:, t, f, 0, 0], y[t, f, 0, 0]) for f in range(F)] for t in range(T)])
    scale = np.maximum(np.abs(exact), np.abs(x.astype(np.float64) - y[None]).mean(axis=0)[..., 0, 0])
    print(f"M = {M} {route}: energy score at d = 1 against crps.crps {np.abs(es - want).max():.3g}, against the integral {np.abs(es - exact).max():.3g}")
    assert np.all(np.abs(es - want) <= 1e-12 * scale) and np.all(np.abs(es - exact) <= 1e-12 * scale)
    if M > 1:
        fair = MV.energy_score(S, Tr, fair=True).numpy()
        assert np.all(np.abs(fair - C.crps(S, Tr, fair=True).numpy()) <= 1e-12 * scale)


def test_the_energy_score_is_non_negative_and_zero_at_the_truth(route):
    x, y = _smooth(6, 3, 2, 8, 8, seed=1)
    for beta in (0.5, 1.0, 1.5):
        es = MV.energy_score(x, y, beta=beta)
        assert torch.all(es >= 0) and torch.all(es > 1e-3)
    same = y[None].expand(6, -1, -1, -1, -1).contiguous()
    assert torch.all(MV.energy_score(same, y) == 0) and torch.all(MV.energy_score(same, y, fair=True) == 0)
    assert torch.all(MV.pair_sqdist(same, y) == 0)


def test_fair_and_plain_differ_by_the_pair_term(route):
    M = 5
    x, y = _smooth(M, 3, 2, 8, 8, seed=2)
    d2 = MV.pair_sqdist(x, y)
    assert d2.shape == (3, 2, M * (M + 1) // 2)
    for beta in (1.0, 0.7):
        b = (d2[..., M:] ** (beta / 2)).sum(dim=-1)
        plain, fair = MV.energy_score(x, y, beta=beta), MV.energy_score(x, y, beta=beta, fair=True)
        assert torch.allclose(plain - fair, b * (1.0 / (M * (M - 1)) - 1.0 / M ** 2), rtol=1e-12, atol=1e-15)
        assert torch.all(fair < plain)
    assert MV.pair_index(M, 0, 1) == 0 and MV.pair_index(M, 0, M) == M - 1 and MV.pair_index(M, 1, 2) == M and MV.pair_index(M, M - 1, M) == M * (M + 1) // 2 - 1


def test_the_joint_score_is_the_score_of_the_concatenated_scaled_vector(route):
    M, T, F, H, W_ = 4, 3, 3, 8, 8
    x, y = _smooth(M, T, F, H, W_, seed=3)
    scale = torch.tensor([0.5, 2.0, 4.0], dtype=torch.float64)  # powers of two: the scaled fields are exact in fp32
    xs, ys = (x / scale.float()[None, None, :, None, None]), (y / scale.float()[None, :, None, None])
    cat_x, cat_y = xs.reshape(M, T, 1, F * H, W_), ys.reshape(T, 1, F * H, W_)
    for fair in (False, True):
        joint = MV.energy_score(x, y, joint=True, scale=scale, fair=fair)
        assert joint.shape == (T,)
        assert torch.allclose(joint, MV.energy_score(cat_x, cat_y, fair=fair)[:, 0], rtol=1e-12, atol=0)
    std = y.double().std(dim=(0, 2, 3), unbiased=False)
    assert torch.allclose(MV.truth_scale(y), std, rtol=1e-12)
    assert torch.allclose(MV.energy_score(x, y, joint=True), MV.energy_score(x, y, joint=True, scale=std), rtol=1e-12, atol=0)


def test_the_variogram_score_sees_dependence_where_the_crps_does_not(route):
    M, T, F, H, W_ = 8, 2, 2, 16, 16
    x, y = _smooth(M, T, F, H, W_, seed=4)
    same = y[None].expand(M, -1, -1, -1, -1).contiguous()
    # on this grid every difference, product and member sum is exact at p = 1 and 2: the score is 0 to the bit.  At p = 0.5 the fp32
    # chain of M equal roots rounds (3 t has 26 bits), and torch's vectorised float64 root and its scalar tail differ in the last bit:
    # 0 within the rule, (2 M + 8) 2^-24 sum (2 g_y)^2, and sum g_y^2 at p = 0.5 is sum g_y at p = 1
    for p in (1.0, 2.0):
        assert torch.all(MV.variogram_score(same, y, radius=2, p=p) == 0)
    w = torch.tensor([1.0 / np.hypot(di, dj) for di, dj in MV.offsets(2)], dtype=torch.float64)
    allow = R.v0_factor(M) * 4.0 * (MV.variogram_terms(same, y, radius=2, p=1.0)[..., 1] * w).sum(-1)
    assert torch.all(MV.variogram_score(same, y, radius=2, p=0.5) <= allow)
    vs, crps = MV.variogram_score(x, y, radius=3), C.crps(x, y)
    # a constant per member: every difference inside a member is unchanged (exactly: the fields lie on a grid of 1 / 64) -- the CRPS moves
    shifted = x + torch.arange(M, dtype=torch.float32).view(M, 1, 1, 1, 1) * 3.0
    assert torch.equal(MV.variogram_score(shifted, y, radius=3), vs) and torch.equal(MV.variogram_terms(shifted, y, radius=3), MV.variogram_terms(x, y, radius=3))
    assert torch.all((C.crps(shifted, y) - crps).abs() > 0.5 * crps)
    # the members' values dealt out anew in every cell: the ensemble of every cell, and with it the CRPS, is what it was; every member
    # is now noise across the field -- the variogram score moves
    g = torch.Generator().manual_seed(0)
    perm = torch.argsort(torch.rand(M, T, F, H, W_, generator=g), dim=0)
    dealt = torch.gather(x, 0, perm)
    assert torch.allclose(C.crps(dealt, y), crps, rtol=1e-12, atol=0)
    moved = MV.variogram_score(dealt, y, radius=3)
    print(f"{route}: variogram score {vs.mean():.4g} -> {moved.mean():.4g} with the members dealt out anew per cell; crps {crps.mean():.4g} both times")
    assert torch.all(moved > 1.2 * vs)
    assert torch.all(MV.energy_score(dealt, y) != MV.energy_score(x, y))


def test_weights_and_variograms_by_lag(route):
    M, T, F, H, W_, Rr = 4, 2, 2, 8, 16, 2
    x, y = _smooth(M, T, F, H, W_, seed=5)
    offs = MV.offsets(Rr)
    assert offs == R.offsets(Rr) and len(offs) == ((2 * Rr + 1) ** 2 - 1) // 2 and offs[:3] == [(0, 1), (0, 2), (1, -2)]
    assert offs == [emu_escore_ops.offset_of(Rr, o) for o in range(len(offs))]
    V = MV.variogram_terms(x, y, radius=Rr)
    assert V.shape == (T, F, len(offs), 3) and V.dtype == torch.float64
    w = torch.tensor([1.0 / np.hypot(di, dj) for di, dj in offs], dtype=torch.float64)
    assert torch.allclose(MV.variogram_score(x, y, radius=Rr), (V[..., 0] * w).sum(-1), rtol=1e-15)
    assert torch.allclose(MV.variogram_score(x, y, radius=Rr, weights="uniform"), V[..., 0].sum(-1), rtol=1e-15)
    one = torch.zeros(len(offs), dtype=torch.float64)
    one[3] = 2.0
    assert torch.allclose(MV.variogram_score(x, y, radius=Rr, weights=one), 2.0 * V[..., 3, 0], rtol=1e-15)
    lag, vy, vx = MV.variogram_by_lag(x, y, radius=Rr, p=1.0)
    V1 = MV.variogram_terms(x, y, radius=Rr, p=1.0)
    dist = sorted({di * di + dj * dj for di, dj in offs})
    assert lag.shape == (len(dist),) and np.allclose(lag.numpy(), np.sqrt(dist)) and vy.shape == vx.shape == (T, F, len(dist))
    counts = MV.pair_counts(Rr, H, W_)
    for k, d in enumerate(dist):
        sel = [o for o, (di, dj) in enumerate(offs) if di * di + dj * dj == d]
        n = sum(counts[o] for o in sel)
        assert torch.allclose(vy[..., k], V1[..., sel, 1].sum(-1) / n, rtol=1e-14) and torch.allclose(vx[..., k], V1[..., sel, 2].sum(-1) / n, rtol=1e-14)
    yd = y.double()
    assert torch.allclose(vy[..., 0], ((yd[..., 1:] - yd[..., :-1]).abs().sum((-2, -1)) + (yd[..., 1:, :] - yd[..., :-1, :]).abs().sum((-2, -1))) /
                          (H * (W_ - 1) + (H - 1) * W_), rtol=1e-6)
    assert torch.all(vx[..., 0] < vx[..., -1])  # a smooth field: the variogram grows with the lag


# ------------------------------------------------------------------------------------------------------------------ both routes

PAIR_SHAPES = [(1, 1, 1, 2, 2), (3, 3, 2, 8, 8), (8, 2, 3, 16, 12), (17, 2, 2, 4, 4), (64, 1, 2, 4, 8), (5, 1, 1, 41, 100), (12, 1, 1, 20, 26)]


@pytest.mark.parametrize("M,T,F,H,W_", PAIR_SHAPES)
def test_pair_distances_of_every_field_kind_against_float64(route, M, T, F, H, W_):
    """hw = 4, 64, 192, 16, 32, 4100 (17 chunks, the last of four cells) and 520; 1, 1, 6, 15, 153, 3 and 10 pair tiles"""
    for kind in R.KINDS:
        x, y, d2 = R.pairs_reference(kind, M, T, F, H * W_)
        S, Tr = _t5(x, y, H, W_)
        got = MV.pair_sqdist(S, Tr)
        assert got.dtype == torch.float64 and got.shape == (T, F, M * (M + 1) // 2)
        r, ok = R.worst_d2(got.numpy(), d2)
        print(f"{route} {kind} {(M, T, F, H * W_)}: D2 error over 3 * 2^-24 D2 (limit 1): {r:.3g}")
        assert ok, (kind, r)
        if kind == "nonfinite":
            assert np.isnan(d2).any() and (T * F == 1 or not np.isnan(d2).all())
        es = MV.energy_score(S, Tr).numpy()
        want = R.energy64(d2, M)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(es), nan) and np.all(np.abs(es - want)[~nan] <= 4 * R.EPS * np.sqrt(np.nan_to_num(d2)).max(axis=-1)[~nan])


def _gram32(x, y):
    """the fast torch route the D2 rule must refuse: |a|^2 + |b|^2 - 2 a.b in fp32"""
    rows = torch.cat([torch.tensor(y)[None], torch.tensor(x)])          # (M + 1, T, F, hw) fp32
    r = rows.permute(1, 2, 0, 3)
    sq = (r * r).sum(-1)
    gram = sq[..., :, None] + sq[..., None, :] - 2.0 * (r @ r.transpose(-1, -2))
    i, j = np.triu_indices(rows.shape[0], 1)
    assert gram.dtype == torch.float32
    return gram[..., i, j].double().numpy()


@pytest.mark.parametrize("M", [3, 8])
def test_the_fp32_gram_form_fails_the_rule_where_the_kernel_s_arithmetic_passes(M, monkeypatch):
    T, F, hw = 2, 2, 256
    x, y, d2 = R.pairs_reference("pressure", M, T, F, hw)
    rg, ok_g = R.worst_d2(_gram32(x, y), d2)
    print(f"pressure M = {M}: fp32 Gram form, D2 error over the bound (limit 1): {rg:.3g}")
    assert not ok_g and rg > 1e3
    emu_escore_ops.install(monkeypatch, escore_ops, MV)
    rk, ok = R.worst_d2(MV.pair_sqdist(*_t5(x, y, 16, 16)).numpy(), d2)
    print(f"pressure M = {M}: the kernel's arithmetic (emulated), D2 error over the bound: {rk:.3g}")
    assert ok and emu_escore_ops.CALLS == [("pairs", M, T * F, hw)]


VARIO_SHAPES = [(1, 2, 1, 8, 8, 1), (2, 1, 2, 16, 24, 3), (8, 1, 2, 24, 16, 3), (9, 1, 1, 40, 8, 8), (16, 1, 1, 8, 40, 2), (3, 2, 1, 16, 72, 8)]


@pytest.mark.parametrize("p", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("M,T,F,H,W_,Rr", VARIO_SHAPES)
def test_variogram_terms_of_every_field_kind_against_float64(route, M, T, F, H, W_, Rr, p):
    """one tile, tiles in both directions, a field narrower than 2 R + 1 and than a tile, 5 tiles in a column, a last tile of 8 columns"""
    for kind in R.KINDS:
        x, y, V, S = R.vario_reference(kind, M, T, F, H, W_, Rr, p)
        got = MV.variogram_terms(torch.tensor(x), torch.tensor(y), radius=Rr, p=p)
        assert got.dtype == torch.float64 and got.shape == V.shape
        r, ok = R.worst_vario(got.numpy(), V, S, M)
        print(f"{route} {kind} {(M, T, F, H, W_)} R = {Rr} p = {p}: error over the rules (limit 1): {r:.3g}")
        assert ok, (kind, r)
        if kind == "nonfinite":
            assert np.isnan(V).any() and (T * F == 1 or not np.isnan(V).all())


def test_one_member_and_no_members(route):
    x, y = _smooth(1, 2, 2, 8, 8, seed=6)
    d2 = MV.pair_sqdist(x, y)
    assert d2.shape == (2, 2, 1)
    assert torch.allclose(MV.energy_score(x, y), torch.sqrt(((x[0] - y).double() ** 2).sum((-2, -1))), rtol=1e-6)  # M = 1: the distance
    assert torch.isnan(MV.energy_score(x, y, fair=True)).all() and not torch.isnan(MV.energy_score(x, y)).any()
    assert not torch.isnan(MV.variogram_score(x, y, radius=2)).any()
    none = x[:0]
    assert MV.pair_sqdist(none, y).shape == (2, 2, 0) and torch.isnan(MV.energy_score(none, y)).all() and MV.energy_score(none, y).shape == (2, 2)
    assert torch.isnan(MV.energy_score(none, y, joint=True)).all()
    assert torch.isnan(MV.variogram_terms(none, y, radius=2)).all() and MV.variogram_terms(none, y, radius=2).shape == (2, 2, 12, 3)
    assert MV.pair_sqdist(x[:, :0], y[:0]).shape == (0, 2, 1) and MV.variogram_terms(x[:, :0], y[:0], radius=1).shape == (0, 2, 4, 3)


def test_a_non_finite_value_poisons_its_own_entries_only(route):
    M, T, F, H, W_, Rr = 5, 3, 2, 8, 8, 2
    x, y = _smooth(M, T, F, H, W_, seed=7)
    clean_d2, clean_v = MV.pair_sqdist(x, y), MV.variogram_terms(x, y, radius=Rr)
    x, y = x.clone(), y.clone()
    x[2, 1, 0, 3, 3] = float("nan")
    x[0, 2, 1, 0, 0] = float("-inf")
    y[0, 1, 7, 7] = float("inf")
    d2, V = MV.pair_sqdist(x, y), MV.variogram_terms(x, y, radius=Rr)
    bad = torch.zeros(T, F, M * (M + 1) // 2, dtype=torch.bool)
    for (t, f), row in (((1, 0), 3), ((2, 1), 1), ((0, 1), 0)):
        for other in range(M + 1):
            if other != row:
                bad[t, f, MV.pair_index(M, min(row, other), max(row, other))] = True
    assert torch.equal(torch.isnan(d2), bad) and torch.equal(d2[~bad], clean_d2[~bad])
    es = MV.energy_score(x, y)
    assert torch.equal(torch.isnan(es), bad.any(-1)) and torch.isnan(MV.energy_score(x, y, joint=True)).all()
    vbad = torch.zeros(T, F, len(MV.offsets(Rr)), dtype=torch.bool)
    for (t, f), (i, j) in (((1, 0), (3, 3)), ((2, 1), (0, 0)), ((0, 1), (7, 7))):
        for o, (di, dj) in enumerate(MV.offsets(Rr)):
            here = i + di < H and 0 <= j + dj < W_
            there = i - di >= 0 and 0 <= j - dj < W_
            vbad[t, f, o] = here or there
    assert torch.equal(torch.isnan(V).all(-1), vbad) and torch.equal(torch.isnan(V).any(-1), vbad)
    assert torch.equal(V[~vbad], clean_v[~vbad])
    assert 0 < int(vbad[2, 1].sum()) < vbad.shape[-1]  # a corner cell: only the offsets that reach into the field
    w = (~vbad[2, 1]).double()
    assert not torch.isnan(MV.variogram_score(x, y, radius=Rr, weights=w)[2, 1])  # an offset of weight 0 is left out


def test_any_dtype_any_strides(route):
    base = 280.0 + 10.0 * torch.randn(4, 3, 2, 8, 32, dtype=torch.float64)
    truth_base = 280.0 + 10.0 * torch.randn(3, 2, 8, 32, dtype=torch.float64)
    view, tview = base[..., ::2], truth_base[..., 1::2]  # strided
    for cast in (torch.float64, torch.float16, torch.bfloat16):
        S, Tr = view.to(cast), tview.to(cast)
        x32, y32 = S.float().numpy(), Tr.float().numpy()
        d2 = R.d2_64(x32.reshape(4, 3, 2, -1), y32.reshape(3, 2, -1))
        assert R.worst_d2(MV.pair_sqdist(S, Tr).numpy(), d2)[1], cast
        V, Sy = R.vario64(x32, y32, 2, 0.5)
        assert R.worst_vario(MV.variogram_terms(S, Tr, radius=2).numpy(), V, Sy, 4)[1], cast


# ------------------------------------------------------------------------------------------------------------------ report

def test_report_keys_and_values(route):
    M, T, F, H, W_ = 4, 3, 2, 8, 16
    x, y = _smooth(M, T, F, H, W_, seed=8)
    rep = MV.multivariate_report(x, y, names=["tas", "psl"], radius=2)
    es, fair, vs = MV.energy_score(x, y), MV.energy_score(x, y, fair=True), MV.variogram_score(x, y, radius=2)
    lag, vy, vx = MV.variogram_by_lag(x, y, radius=2)
    assert rep.names == ["tas", "psl"] and torch.equal(rep.lag, lag)
    for f, (name, v) in enumerate(rep):
        assert set(v) == {"energy", "energy_fair", "variogram", "energy_by_time", "variogram_by_time", "variogram_truth", "variogram_ensemble"}
        assert rep[name] is v and all(t.dtype == torch.float64 for t in v.values()) and v["energy"].dim() == 0 and v["energy_by_time"].shape == (T,)
        assert torch.equal(v["energy_by_time"], es[:, f]) and torch.equal(v["variogram_by_time"], vs[:, f])
        assert float(v["energy"]) == pytest.approx(float(es[:, f].mean()), rel=1e-14) and float(v["energy_fair"]) == pytest.approx(float(fair[:, f].mean()), rel=1e-14)
        assert float(v["variogram"]) == pytest.approx(float(vs[:, f].mean()), rel=1e-14)
        assert torch.allclose(v["variogram_truth"], vy[:, f].mean(0), rtol=1e-13) and torch.allclose(v["variogram_ensemble"], vx[:, f].mean(0), rtol=1e-13)
    joint = MV.energy_score(x, y, joint=True)
    assert torch.equal(rep.joint["energy_by_time"], joint) and float(rep.joint["energy"]) == pytest.approx(float(joint.mean()), rel=1e-14)
    flat = rep.as_dict()
    assert set(flat) == {f"multivariate/{n}/{k}" for n in ("tas", "psl") for k in ("energy", "energy_fair", "variogram")} | {
        "multivariate/joint/energy", "multivariate/joint/energy_fair"}
    assert all(isinstance(val, float) for val in flat.values())
    assert flat["multivariate/psl/variogram"] == float(rep["psl"]["variogram"]) and flat["multivariate/joint/energy_fair"] == float(rep.joint["energy_fair"])
    assert set(rep.as_dict("eval")) >= {"eval/tas/energy"} and MV.multivariate_report(x, y).names == ["var0", "var1"]


def test_argument_checks():
    x, y = torch.zeros(3, 2, 2, 8, 8), torch.zeros(2, 2, 8, 8)
    calls = (MV.pair_sqdist, MV.energy_score, lambda a, b: MV.variogram_terms(a, b, radius=1), lambda a, b: MV.variogram_score(a, b, radius=1),
             lambda a, b: MV.variogram_by_lag(a, b, radius=1), MV.multivariate_report)
    for fn in calls:
        with pytest.raises(ValueError, match=r"\(3, 2, 2, 8, 4\)"):
            fn(x[..., :4], y)
        with pytest.raises(ValueError):
            fn(x[0], y)
        with pytest.raises(ValueError):
            fn(x, y[0])
        with pytest.raises(ValueError):
            fn(x.long(), y)
    for beta in (0.0, 2.0, -1.0):
        with pytest.raises(ValueError, match="beta"):
            MV.energy_score(x, y, beta=beta)
    with pytest.raises(ValueError, match="joint=True"):
        MV.energy_score(x, y, scale=[1.0, 1.0])
    with pytest.raises(ValueError, match="3 entries for 2 variables"):
        MV.energy_score(x, y, joint=True, scale=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="radius"):
        MV.variogram_terms(x, y, radius=0)
    with pytest.raises(ValueError, match="order"):
        MV.variogram_terms(x, y, radius=1, p=0.0)
    with pytest.raises(ValueError, match="weights"):
        MV.variogram_score(x, y, radius=1, weights="gaussian")
    with pytest.raises(ValueError, match=r"\(4,\)"):
        MV.variogram_score(x, y, radius=1, weights=torch.ones(5))
    with pytest.raises(ValueError, match="1 names for 2 variables"):
        MV.multivariate_report(x, y, names=["only_one"])


def test_unsupported_shapes_take_the_general_route(monkeypatch):
    """hw no multiple of 4 and M > 64; H no multiple of 8, R = 9, M = 17 and p = 0.75: the launcher is asked, answers no, nothing is
    launched, the general route answers"""
    emu_escore_ops.install(monkeypatch, escore_ops, MV)
    for M, H, W_ in ((3, 5, 5), (65, 2, 2)):
        x, y = CR.fields("wind", M, 2, 2, H * W_)
        got = MV.pair_sqdist(*_t5(x, y, H, W_))
        assert np.allclose(got.numpy(), R.d2_64(x, y), rtol=1e-13, atol=0)
    for M, H, W_, Rr, p in ((3, 12, 8, 2, 0.5), (3, 8, 8, 9, 0.5), (17, 8, 8, 2, 0.5), (3, 8, 8, 2, 0.75), (2, 5, 7, 3, 1.0)):
        x, y = R.fields("wind", M, 1, 2, H, W_)
        V, _ = R.vario64(x, y, Rr, p)
        got = MV.variogram_terms(torch.tensor(x), torch.tensor(y), radius=Rr, p=p)
        assert np.allclose(got.numpy(), V, rtol=1e-12, atol=1e-300)
    assert emu_escore_ops.CALLS == []  # *_supported said no before anything was allocated
    assert not emu_escore_ops.escore_pairs(None, None, None, None, 65, 4, 16) and not emu_escore_ops.escore_pairs(None, None, None, None, 3, 4, 6)
    assert not emu_escore_ops.vario_terms(None, None, None, None, 17, 2, 8, 8, 2, 1) and not emu_escore_ops.vario_terms(None, None, None, None, 3, 2, 8, 8, 9, 1)


# ------------------------------------------------------------------------------------------------------------------ the kernels' maps

@pytest.fixture(scope="module")
def host_escore(tmp_path_factory):
    """a stand-alone program under the address and undefined-behaviour sanitizers; it is run directly, never loaded into Python.
    -ffp-contract=off: the kernels fuse no multiply with an add either (escore_core.h says so to its own compiler)."""
    return host_program.build(tmp_path_factory, "escore", sanitize=True, fp_contract_off=True, timeout=600)


@pytest.mark.parametrize("M,planes,hw", [(1, 2, 4), (2, 3, 64), (3, 2, 260), (7, 4, 192), (8, 2, 1028), (16, 2, 516), (33, 1, 260), (64, 2, 4100)])
def test_every_cell_of_every_plane_is_fetched_exactly_once(host_escore, M, planes, hw):
    """planes smaller than a chunk, of one chunk + 4 cells and of 16 chunks + 4; 1 to 153 pair tiles.  The fields hold their own
    indices, so what a workgroup staged says where from; the program also asserts that every pair of every chunk was written"""
    rc = subprocess.run([str(host_escore), "visit_pairs", str(M), str(planes), str(hw)], timeout=600).returncode
    assert rc == 0, f"check {rc} of host_escore_main.cpp failed"


@pytest.mark.parametrize("M,planes,H,W_,Rr", [(1, 2, 8, 8, 1), (2, 3, 16, 24, 3), (3, 2, 24, 16, 8), (16, 1, 40, 8, 8), (2, 1, 8, 72, 8), (4, 2, 16, 40, 5)])
def test_every_in_field_pair_of_every_offset_is_visited_exactly_once(host_escore, M, planes, H, W_, Rr):
    """one tile and several in either direction, a last tile of 8 columns, fields narrower than 2 R + 1; and no pair with a cell outside
    the field is taken up"""
    rc = subprocess.run([str(host_escore), "visit_vario", str(M), str(planes), str(H), str(W_), str(Rr)], timeout=600).returncode
    assert rc == 0, f"check {rc} of host_escore_main.cpp failed"


@pytest.mark.parametrize("M,T,F,hw", [(1, 2, 1, 8), (3, 2, 2, 64), (8, 1, 2, 260), (12, 1, 1, 516), (17, 1, 1, 4100), (64, 1, 1, 260)])
def test_pairs_on_the_host_equal_the_emulation_bit_for_bit(host_escore, tmp_path, M, T, F, hw):
    """csrc/escore_core.h compiled for the host against tests/emu_escore_ops.py: the tiles, the slices, the arithmetic, the fold through
    LDS and over the chunks; every kind"""
    for kind in R.KINDS:
        x, y = CR.fields(kind, M, T, F, hw)
        x.tofile(tmp_path / "x"), y.tofile(tmp_path / "y")
        d2 = torch.full((T, F, M * (M + 1) // 2), -7.25, dtype=torch.float64)
        nbytes = emu_escore_ops.escore_scratch_bytes(T * F, hw, M)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64) if nbytes else None
        assert emu_escore_ops.escore_pairs(torch.tensor(x), torch.tensor(y), d2, scratch, M, T * F, hw)
        subprocess.run([str(host_escore), "pairs", str(M), str(T * F), str(hw)] + [str(tmp_path / n) for n in ("x", "y", "d2")], check=True, timeout=600)
        assert _same_bits(np.fromfile(tmp_path / "d2", dtype=np.float64).reshape(d2.shape), d2.numpy()), kind


@pytest.mark.parametrize("M,planes,H,W_,Rr,order2", [(1, 2, 8, 8, 1, 1), (2, 1, 16, 24, 3, 2), (8, 2, 24, 16, 3, 4), (9, 1, 40, 8, 8, 1), (16, 1, 8, 40, 2, 1)])
def test_variogram_terms_on_the_host_equal_the_emulation_bit_for_bit(host_escore, tmp_path, M, planes, H, W_, Rr, order2):
    for kind in R.KINDS:
        x, y = R.fields(kind, M, planes, 1, H, W_)
        x.tofile(tmp_path / "x"), y.tofile(tmp_path / "y")
        V = torch.full((planes, emu_escore_ops.n_offsets(Rr), 3), -7.25, dtype=torch.float64)
        nbytes = emu_escore_ops.vario_scratch_bytes(planes, H, W_, Rr)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64) if nbytes else None
        assert emu_escore_ops.vario_terms(torch.tensor(x), torch.tensor(y), V, scratch, M, planes, H, W_, Rr, order2)
        subprocess.run([str(host_escore), "vario", str(M), str(planes), str(H), str(W_), str(Rr), str(order2)] + [str(tmp_path / n) for n in ("x", "y", "V")],
                       check=True, timeout=600)
        assert _same_bits(np.fromfile(tmp_path / "V", dtype=np.float64).reshape(V.shape), V.numpy()), kind


def test_support_predicates_and_maps_agree():
    for hw, M, want in ((4, 1, True), (16384, 64, True), (6, 8, False), (64, 65, False), (64, 0, False), (0, 8, False)):
        assert emu_escore_ops.escore_supported(hw, M) is want
    for H, W_, Rr, M, o2, want in ((8, 8, 1, 1, 1, True), (128, 128, 8, 16, 4, True), (12, 8, 1, 1, 1, False), (8, 8, 9, 1, 1, False), (8, 8, 0, 1, 1, False),
                                   (8, 8, 1, 17, 1, False), (8, 8, 1, 0, 1, False), (8, 8, 1, 1, 3, False)):
        assert emu_escore_ops.vario_supported(H, W_, Rr, M, o2) is want
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "escore_core.h")).read()
    shared = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "ordered_sum.h")).read()
    for text in ("THREADS = 256", "GROUP = 16"):
        assert text in shared, text
    for text in ("THREADS = 256", "P_MAX_M = 64", "P_CHUNK = 256", "P_PITCH = P_CHUNK + 4", "V_MAX_M = 16", "V_MAX_R = 8", "V_TH = 8, V_TW = 32",
                 "V_BATCH = 4", "hw >= 4 && hw % 4 == 0 && M >= 1 && M <= P_MAX_M", "H % 8 == 0 && W % 8 == 0 && R >= 1 && R <= V_MAX_R && M >= 1 && M <= V_MAX_M"):
        assert text in core, text
    assert [emu_escore_ops.tiles(M) for M in (1, 3, 4, 7, 8, 16, 33, 64)] == [1, 1, 3, 3, 6, 15, 45, 153]
    assert [emu_escore_ops.slices(M) for M in (1, 3, 4, 7, 8, 16, 33, 64)] == [64, 64, 64, 64, 32, 16, 4, 1]
    assert emu_escore_ops.lds_bytes(64) == 67600 and emu_escore_ops.lds_bytes(8) == 32768
    assert emu_escore_ops.vario_lds_bytes(8, 16) == 78336 and emu_escore_ops.vario_lds_bytes(1, 1) == 2 * 9 * 34 * 4 + 26112
    assert all(emu_escore_ops.n_offsets(Rr) % 4 == 0 for Rr in range(1, 9))  # the kernel walks the offsets four at a time
    assert emu_escore_ops.escore_scratch_bytes(6, 16384, 8) == 6 * 64 * 36 * 8 and emu_escore_ops.escore_scratch_bytes(6, 256, 8) == 0
    assert emu_escore_ops.vario_scratch_bytes(6, 128, 128, 4) == 6 * 64 * 40 * 3 * 8 and emu_escore_ops.vario_scratch_bytes(6, 8, 32, 4) == 0


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_escore_supported": "int", "c2w_escore_scratch_bytes": "long long", "c2w_escore_pairs": "int",
             "c2w_vario_supported": "int", "c2w_vario_scratch_bytes": "long long", "c2w_vario_terms": "int"}
    c_abi.assert_declared(names, "escore.hip", escore_ops, ("escore_supported", "escore_scratch_bytes", "escore_pairs", "vario_supported", "vario_scratch_bytes", "vario_terms"))
