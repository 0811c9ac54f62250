"""CPU checks of the event verification (climate2weather_amd.events): both routes of the two tables -- the general torch one and the
launcher's, with tests/emu_event_ops.py standing in for the HIP kernels -- EQUAL to the NumPy reference of tests/fp64_events_ref.py on
every kind of field; the known answers, all exact -- a forecast equal to the truth, one displaced cell, an all-event plane, a constant
forecast, the radius-0 row against the joint table; the identities of the Brier decomposition; the fair score by a seeded Monte-Carlo
draw with its own standard error; the box filter against scipy.ndimage.uniform_filter(mode="constant"); NaN cells; every ValueError;
the kernels' own index maps and arithmetic compiled for the host (csrc/events_core.h), once plain and once under the address and
undefined-behaviour sanitizers; and the C declarations against the ctypes prototypes."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_event_ops
import fp64_events_ref as R
import host_program
from climate2weather_amd import event_ops
from climate2weather_amd import events as EV
from climate2weather_amd.ensemble_host import VariableReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of events.event_counts / events.fss_sums on CPU tensors"""
    if request.param == "launcher":
        emu_event_ops.install(monkeypatch, event_ops, EV)
    return request.param


def _case(kind, M, T, F, H, W_, K, direction="mixed", seed=0):
    """the arrays of the reference and the tensors of the public interface"""
    x, y = R.fields(kind, M, T, F, H * W_, seed)
    thr, above = R.thresholds(kind, y, K), R.directions(F, K, direction)
    return x, y, thr, above, torch.tensor(x).view(M, T, F, H, W_), torch.tensor(y).view(T, F, H, W_), torch.tensor(thr), R.direction_names(above)


def _planes(truth_plane, member_planes):
    """(H, W) and M x (H, W) indicator arrays -> samples (M, 1, 1, H, W), truth (1, 1, H, W) fp32 with the event at values >= 1"""
    return torch.tensor(np.stack(member_planes), dtype=torch.float32)[:, None, None], torch.tensor(truth_plane, dtype=torch.float32)[None, None]


ONE = torch.tensor([[1.0]])


# ------------------------------------------------------------------------------------------------------------------ against the reference

@pytest.mark.parametrize("H,W_,M,K", [(1, 4, 1, 1), (2, 6, 3, 2), (41, 100, 9, 3), (8, 8, 2, 8)])
def test_the_joint_table_equals_the_reference(route, H, W_, M, K):
    """hw = 4, 12, 4100 (two chunks) and 64; hw = 12 at H W not a multiple of 4 in W alone; every kind, mixed directions"""
    for i, kind in enumerate(R.KINDS):
        x, y, thr, above, S, Tr, th, names = _case(kind, M, 2, 2, H, W_, K, ("mixed", "above", "below")[i % 3])
        counts, invalid = EV.event_counts(S, Tr, th, names)
        want, winv = R.counts_ref(x, y, thr, above)
        assert counts.dtype == torch.int64 and counts.shape == (2, 2, K, 2, M + 1) and invalid.shape == (2, 2)
        assert np.array_equal(counts.numpy(), want) and np.array_equal(invalid.numpy(), winv), kind
        assert np.array_equal(counts.sum(dim=(-1, -2)).numpy() + invalid.numpy()[:, :, None], np.full((2, 2, K), H * W_))
    if route == "launcher":
        assert emu_event_ops.CALLS and all(c[0] == "counts" for c in emu_event_ops.CALLS)


@pytest.mark.parametrize("H,W_,M,radii", [(4, 4, 1, (0,)), (8, 12, 3, (0, 1, 2, 16)), (68, 72, 2, (0, 3, 16)), (7, 9, 2, (0, 2, 40))])
def test_the_fss_sums_equal_the_reference(route, H, W_, M, radii):
    """planes whose every window is clipped, remainder tiles of width 4 and 8, and a shape only the general route takes"""
    for i, kind in enumerate(R.KINDS if H < 60 else R.KINDS[::3]):
        x, y, thr, above, S, Tr, th, names = _case(kind, M, 2, 2, H, W_, 2, ("mixed", "above", "below")[i % 3])
        sums = EV.fss_sums(S, Tr, th, radii, names)
        assert sums.dtype == torch.int64 and sums.shape == (2, 2, 2, len(radii), M + 2, 2)
        assert np.array_equal(sums.numpy(), R.fss_ref(x, y, thr, above, radii, H, W_)), kind
        assert torch.equal(sums[..., 0, 0], sums[..., 0, 1])  # the truth's row holds (OO, OO)


def test_the_launcher_declines_what_the_kernels_do_not_take(monkeypatch):
    emu_event_ops.install(monkeypatch, event_ops, EV)
    x, y, thr, above, S, Tr, th, names = _case("wind", 2, 1, 1, 3, 6, 2)
    c, _ = EV.event_counts(S, Tr, th, names)           # hw = 18
    s = EV.fss_sums(S, Tr, th, (0, 1), names)          # W = 6
    assert np.array_equal(c.numpy(), R.counts_ref(x, y, thr, above)[0]) and np.array_equal(s.numpy(), R.fss_ref(x, y, thr, above, (0, 1), 3, 6))
    assert [c_[0] for c_ in emu_event_ops.CALLS] == []  # *_supported said no before a launcher was reached
    assert not emu_event_ops.counts_supported(18, 2, 2) and not emu_event_ops.counts_supported(16, 65, 2) and not emu_event_ops.counts_supported(16, 2, 9)
    assert emu_event_ops.counts_supported(4, 1, 1) and emu_event_ops.counts_supported(16384, 64, 8)
    assert not emu_event_ops.fss_supported(3, 8, 2, 2, (0,)) and not emu_event_ops.fss_supported(8, 6, 2, 2, (0,))
    assert not emu_event_ops.fss_supported(8, 8, 2, 2, (17,)) and not emu_event_ops.fss_supported(8, 8, 2, 2, range(9))
    assert not emu_event_ops.fss_supported(1024, 1028, 2, 2, (0,)) and emu_event_ops.fss_supported(1024, 1024, 64, 8, (0, 16))
    assert emu_event_ops.fss_no_overflow(1024, 1024, 64, 16) and not emu_event_ops.fss_no_overflow(1 << 15, 1 << 15, 64, 16)


def test_the_general_route_chunked_over_time_gives_the_same_tables(monkeypatch):
    monkeypatch.setattr(EV, "chunk_step", lambda per_item: 2)  # 7 times in chunks of 2: the last chunk is short
    x, y, thr, above, S, Tr, th, names = _case("nans", 3, 7, 2, 8, 12, 2)
    counts, invalid = EV.event_counts(S, Tr, th, names)
    want, winv = R.counts_ref(x, y, thr, above)
    assert np.array_equal(counts.numpy(), want) and np.array_equal(invalid.numpy(), winv)
    assert np.array_equal(EV.fss_sums(S, Tr, th, (0, 1, 3), names).numpy(), R.fss_ref(x, y, thr, above, (0, 1, 3), 8, 12))


def test_strided_and_half_precision_inputs_and_float64_thresholds(route):
    g = torch.Generator().manual_seed(3)
    base = (torch.randn(3, 2, 2, 8, 16, generator=g) * 2.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]
    thr64 = torch.tensor([[0.1, 1.3], [-0.7, 0.9]], dtype=torch.float64)
    a = EV.event_counts(view, truth, thr64)
    b = EV.event_counts(view.float().contiguous(), truth.float().contiguous(), thr64.float())  # rounded once to fp32
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(EV.fss_sums(view, truth, thr64, (0, 2)), EV.fss_sums(view.float().contiguous(), truth.float().contiguous(), thr64.float(), (0, 2)))


# ------------------------------------------------------------------------------------------------------------------ known answers

def test_a_forecast_equal_to_the_truth_is_perfect(route):
    g = torch.Generator().manual_seed(1)
    truth = torch.randn(3, 2, 12, 16, generator=g)
    samples = truth[None].expand(4, -1, -1, -1, -1).contiguous()
    thr = torch.tensor([[0.0, 1.0], [-0.5, 0.5]])
    counts, invalid = EV.event_counts(samples, truth, thr)
    member, ens = EV.fss(EV.fss_sums(samples, truth, thr, (0, 1, 2, 16)))
    assert torch.equal(member, torch.ones_like(member)) and torch.equal(ens, torch.ones_like(ens))
    assert torch.equal(EV.brier_score(counts), torch.zeros(3, 2, 2, dtype=torch.float64))
    assert torch.equal(EV.roc_area(counts), torch.ones(3, 2, 2, dtype=torch.float64)) and int(invalid.sum()) == 0
    assert torch.equal(EV.brier_skill_score(counts), torch.ones(3, 2, 2, dtype=torch.float64))


@pytest.mark.parametrize("r,d,want", [(2, 1, 0.8), (2, 5, 0.0), (16, 16, 17.0 / 33.0), (1, 2, 1.0 / 3.0), (0, 1, 0.0)])
@pytest.mark.parametrize("axis", [0, 1])
def test_one_displaced_cell_gives_one_minus_d_over_the_window(route, r, d, want, axis):
    """one event cell in the truth and one in the member, d cells apart along an axis, far from the border: the windows overlap in
    (2r + 1)(2r + 1 - d) cells, FSS = 1 - d / (2r + 1), and 0 from d >= 2r + 1"""
    H = W_ = 80
    truth, member = np.zeros((H, W_)), np.zeros((H, W_))
    truth[30, 28] = 1
    member[(30 + d, 28) if axis == 0 else (30, 28 + d)] = 1
    S, Tr = _planes(truth, [member])
    member_fss, ens = EV.fss(EV.fss_sums(S, Tr, ONE, (r,)))
    assert member_fss.item() == want and ens.item() == want and member_fss.item() == max(0, 2 * r + 1 - d) / (2 * r + 1)  # 1 - d / (2r + 1) as one quotient


@pytest.mark.parametrize("H,W_,r", [(4, 8, 8), (5, 4, 16), (12, 20, 3), (68, 72, 16)])
def test_an_all_event_plane_has_the_product_of_the_clipped_extents(route, H, W_, r):
    S, Tr = _planes(np.ones((H, W_)), [np.ones((H, W_))] * 2)
    sums = EV.fss_sums(S, Tr, ONE, (r,))
    a = [min(i + r + 1, H) - max(i - r, 0) for i in range(H)]
    b = [min(j + r + 1, W_) - max(j - r, 0) for j in range(W_)]
    want = sum(v * v for v in a) * sum(v * v for v in b)
    assert sums[0, 0, 0, 0, :3].tolist() == [[want, want]] * 3 and sums[0, 0, 0, 0, 3].tolist() == [4 * want, 2 * want]
    if H <= r and W_ <= r:
        assert want == (H * W_) ** 3


def test_the_radius_zero_ensemble_row_is_the_joint_table(route):
    """sum j^2 N = PP, sum j o N = PO, sum o N = OO, and so the Brier score follows from either kernel"""
    x, y, thr, above, S, Tr, th, names = _case("temperature", 5, 3, 2, 8, 12, 3)
    counts, _ = EV.event_counts(S, Tr, th, names)
    sums = EV.fss_sums(S, Tr, th, (1, 0), names)[:, :, :, 1]
    j, o = torch.arange(6).view(1, 6), torch.arange(2).view(2, 1)
    assert torch.equal((counts * j * j).sum(dim=(-1, -2)), sums[..., 6, 0])
    assert torch.equal((counts * j * o).sum(dim=(-1, -2)), sums[..., 6, 1])
    assert torch.equal((counts * o).sum(dim=(-1, -2)), sums[..., 0, 0])
    pp, po, oo = (sums[..., 6, 0].double(), sums[..., 6, 1].double(), sums[..., 0, 0].double())
    assert torch.allclose(EV.brier_score(counts), (pp / 25 - 2 * po / 5 + oo) / 96, rtol=1e-13, atol=1e-15)
    table = EV.member_contingency(EV.fss_sums(S, Tr, th, (1, 0), names), (1, 0), 96)
    e, ey = R.indicator(x, thr, above), R.indicator(y, thr, above)
    assert np.array_equal(table["hits"].numpy(), np.moveaxis((e & ey).sum(-1), 0, -1))
    assert np.array_equal(table["false_alarms"].numpy(), np.moveaxis((e & ~ey).sum(-1), 0, -1))
    assert np.array_equal(table["misses"].numpy(), np.moveaxis((~e & ey).sum(-1), 0, -1))
    assert np.array_equal(table["correct_negatives"].numpy(), np.moveaxis((~e & ~ey).sum(-1), 0, -1))
    assert np.array_equal(table["frequency_bias"].numpy(), np.moveaxis(e.sum(-1) / ey.sum(-1), 0, -1))
    assert np.array_equal(table["csi"].numpy(), np.moveaxis((e & ey).sum(-1) / (e | ey).sum(-1), 0, -1))


def test_a_nan_cell_is_in_no_bin_and_is_counted(route):
    x, y, thr, above, S, Tr, th, names = _case("wind", 3, 2, 2, 4, 8, 2)
    clean, none = EV.event_counts(S, Tr, th, names)
    S, Tr = S.clone(), Tr.clone()
    S[1, 0, 1, 2, 3] = float("nan")
    Tr[1, 0, 0, 7] = float("nan")
    S[0, 1, 0, 0, 7] = float("nan")    # the same cell as the truth's: one invalid cell, not two
    counts, invalid = EV.event_counts(S, Tr, th, names)
    assert int(none.sum()) == 0 and invalid.tolist() == [[0, 1], [1, 0]]
    assert torch.equal(counts[0, 0], clean[0, 0]) and torch.equal(counts[1, 1], clean[1, 1])
    assert torch.equal(counts.sum(dim=(-1, -2)), 32 - invalid[:, :, None].expand(2, 2, 2))
    xs, ys = S.view(3, 2, 2, 32).numpy(), Tr.view(2, 2, 32).numpy()
    assert np.array_equal(counts.numpy(), R.counts_ref(xs, ys, thr, above)[0])
    # in the FSS a NaN is no event in its own row and the cell stays
    assert np.array_equal(EV.fss_sums(S, Tr, th, (0, 1), names).numpy(), R.fss_ref(xs, ys, thr, above, (0, 1), 4, 8))


# ------------------------------------------------------------------------------------------------------------------ the algebra

def _random_counts(seed, lead=(3, 2), M=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 500, lead + (2, M + 1), generator=g)


def test_the_brier_score_is_reliability_less_resolution_plus_uncertainty():
    for seed, M in ((0, 1), (1, 7), (2, 64)):
        counts = _random_counts(seed, M=M)
        counts[0, 0, :, 2 % (M + 1)] = 0  # an empty bin adds nothing
        rel, res, unc = EV.brier_decomposition(counts)
        bs = EV.brier_score(counts)
        assert torch.all((bs - (rel - res + unc)).abs() <= 1e-12)
        N = counts.double().numpy()
        p = np.arange(M + 1) / M
        want = ((N[..., 0, :] * p ** 2).sum(-1) + (N[..., 1, :] * (p - 1) ** 2).sum(-1)) / N.sum((-1, -2))
        assert np.allclose(bs.numpy(), want, rtol=1e-14, atol=0)
        assert np.allclose(EV.brier_skill_score(counts).numpy(), 1 - want / unc.numpy(), rtol=1e-13, atol=0)
    only = torch.zeros(2, 4, dtype=torch.int64)
    only[0] = torch.tensor([5, 1, 0, 2])       # the truth never has the event
    assert math.isnan(EV.brier_skill_score(only).item()) and EV.brier_decomposition(only)[2].item() == 0.0
    assert math.isnan(EV.brier_skill_score(only.flip(0)).item())


def test_the_fair_score_of_a_constant_probability_forecast_averages_to_p_minus_o_squared():
    """members drawn independently with probability p = 0.3 where the truth has no event: the fair score averages to (p - o)^2 = 0.09
    whatever M.  The standard error follows from the binomial law of j, not from the draw."""
    M, p, n = 5, 0.3, 400_000
    rng = np.random.default_rng(20260)
    j = rng.binomial(M, p, size=n)
    counts = torch.zeros(2, M + 1, dtype=torch.int64)
    counts[0] = torch.tensor(np.bincount(j, minlength=M + 1))
    pmf = np.array([math.comb(M, k) * p ** k * (1 - p) ** (M - k) for k in range(M + 1)])
    score = (np.arange(M + 1) / M) ** 2 - np.arange(M + 1) * (M - np.arange(M + 1)) / (M * M * (M - 1))
    mean, var = (pmf * score).sum(), (pmf * score ** 2).sum() - (pmf * score).sum() ** 2
    assert abs(mean - 0.09) < 1e-15                   # the correction is unbiased, exactly
    se = math.sqrt(var / n)
    got = EV.brier_score(counts, fair=True).item()
    print(f"fair Brier score {got:.5f} against 0.09, standard error {se:.2e}")
    assert abs(got - 0.09) <= 5 * se and EV.brier_score(counts).item() > 0.09 + 20 * se  # the plain score is biased by p (1 - p) / M
    assert math.isnan(EV.brier_score(torch.ones(2, 2, dtype=torch.int64), fair=True).item())  # M = 1


def test_the_roc_of_a_constant_forecast_and_of_a_known_table():
    M = 4
    for j in range(M + 1):
        counts = torch.zeros(2, M + 1, dtype=torch.int64)
        counts[0, j], counts[1, j] = 70, 30
        assert EV.roc_area(counts).item() == 0.5
    counts = torch.tensor([[6, 3, 1], [1, 2, 7]])      # M = 2
    hit, fa = EV.roc_curve(counts)
    assert hit.tolist() == [1.0, 0.9, 0.7, 0.0] and fa.tolist() == [1.0, 0.4, 0.1, 0.0]
    assert abs(EV.roc_area(counts).item() - (0.6 * 0.95 + 0.3 * 0.8 + 0.1 * 0.35)) <= 1e-15
    prob, freq, n = EV.reliability_curve(counts)
    assert prob.tolist() == [0.0, 0.5, 1.0] and freq.tolist() == [1 / 7, 2 / 5, 7 / 8] and n.tolist() == [7, 5, 8]
    with pytest.raises(ValueError, match=r"must be \(\.\.\., 2, M \+ 1\)"):
        EV.roc_curve(torch.zeros(3, 4))


def test_the_fss_agrees_with_the_uniform_filter_form():
    """the zero-padded box filter of scipy.ndimage: fractions P = uniform_filter(indicator, 2r + 1, mode="constant"),
    FSS = 1 - sum (P_f - P_o)^2 / (sum P_f^2 + sum P_o^2), for a member and for the ensemble probability"""
    from scipy import ndimage
    H, W_, M, radii = 40, 52, 3, (0, 1, 2, 7, 16)
    x, y, thr, above, S, Tr, th, names = _case("wind", M, 1, 1, H, W_, 1, "above")
    sums = EV.fss_sums(S, Tr, th, radii, names)
    member, ens = EV.fss(sums)
    e = R.indicator(x, thr, above).reshape(M, H, W_).astype(np.float64)
    o = R.indicator(y, thr, above).reshape(H, W_).astype(np.float64)
    worst = 0.0
    for s, r in enumerate(radii):
        box = lambda a: ndimage.uniform_filter(a, size=2 * r + 1, mode="constant", cval=0.0)
        po = box(o)
        for m, field in list(enumerate(e)) + [(M, e.mean(axis=0))]:
            pf = box(field)
            want = 1.0 - ((pf - po) ** 2).sum() / ((pf ** 2).sum() + (po ** 2).sum())
            got = (member[0, 0, 0, s, m] if m < M else ens[0, 0, 0, s]).item()
            worst = max(worst, abs(got - want))
    print(f"FSS against the uniform_filter form: worst difference {worst:.3g}")
    assert worst <= 1e-12


def test_pooling_sums_the_integers_first_and_the_useful_scale_is_the_first_radius_that_reaches_it(route):
    H = W_ = 40
    truth, member = np.zeros((2, H, W_)), np.zeros((2, H, W_))
    truth[0, 20, 20] = truth[1, 10, 10] = 1
    member[0, 20, 23] = member[1, 10, 10] = 1       # time 0 displaced by 3, time 1 exact
    S = torch.tensor(member, dtype=torch.float32)[None, :, None]
    Tr = torch.tensor(truth, dtype=torch.float32)[:, None]
    radii = (0, 1, 2, 4)
    sums = EV.fss_sums(S, Tr, ONE, radii)
    per_time = EV.fss(sums)[1][:, 0, 0]
    assert per_time[0].tolist() == [0.0, 0.0, 0.4, 6.0 / 9.0] and per_time[1].tolist() == [1.0] * 4
    pooled = EV.fss(sums, pooled=True)[1][0, 0]
    assert pooled.tolist() == [0.5, 0.5, 0.7, (2 * 54.0 + 2 * 81.0) / (4 * 81.0)]
    assert EV.fss_useful_scale(sums, radii, H * W_).tolist() == [[2]]   # f0 = 1 / 1600: the target is just above 0.5, which radius 1 only equals
    assert EV.fss_useful_scale(sums[:1], radii, H * W_).tolist() == [[4]] and EV.fss_useful_scale(sums[:1, :, :, :3], radii[:3], H * W_).tolist() == [[-1]]
    empty = EV.fss(EV.fss_sums(torch.zeros_like(S), torch.zeros_like(Tr), ONE, radii))
    assert torch.isnan(empty[0]).all() and torch.isnan(empty[1]).all()


def test_thresholds_from_quantiles_and_the_report(route):
    x, y, thr, above, S, Tr, th, names = _case("pressure", 4, 3, 2, 8, 12, 2, "above")
    got = EV.thresholds_from_quantiles(Tr, (0.5, 0.9))
    want = np.quantile(y.astype(np.float64).transpose(1, 0, 2).reshape(2, -1), [0.5, 0.9], axis=1).T.astype(np.float32)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    rep = EV.events_report(S, Tr, levels=(0.5, 0.9), radii=(0, 1, 2), names=["psl", "tas"])
    assert isinstance(rep, VariableReport) and rep.names == ["psl", "tas"]
    counts, invalid = EV.event_counts(S, Tr, got)
    sums = EV.fss_sums(S, Tr, got, (0, 1, 2))
    C = counts.sum(dim=0)
    for f, (name, v) in enumerate(rep):
        assert torch.equal(v["thresholds"], got[f]) and torch.equal(v["brier"], EV.brier_score(C[f]))
        assert torch.equal(v["brier_fair"], EV.brier_score(C[f], fair=True)) and torch.equal(v["roc_area"], EV.roc_area(C[f]))
        rel, res, unc = EV.brier_decomposition(C[f])
        assert torch.equal(v["reliability"], rel) and torch.equal(v["resolution"], res) and torch.equal(v["uncertainty"], unc)
        assert torch.equal(v["fss"], EV.fss(sums, pooled=True)[1][f]) and torch.equal(v["fss_member"], EV.fss(sums, pooled=True)[0][f])
        assert torch.equal(v["fss_time"], EV.fss(sums)[1][:, f]) and v["fss_useful_scale"].shape == (2,)
        assert torch.equal(v["hits"], sums[:, f, :, 0, 1:5, 1].sum(dim=0)) and int(v["invalid"]) == 0
        assert abs(v["base_rate"][0].item() - 0.5) < 0.01 and v["hit_rate"].shape == (2, 6)
    flat = rep.as_dict()
    assert set(flat) == {f"events/{n}/fss_k{k}_r{r}{s}" for n in ("psl", "tas") for k in (0, 1) for r in (0, 1, 2) for s in ("", "_std")}
    assert flat["events/psl/fss_k0_r1"] == pytest.approx(rep["psl"]["fss_member"][0, 1].mean().item(), abs=1e-15)
    explicit = EV.events_report(S, Tr, thresholds=got, radii=(1, 2), direction="below")
    assert "hits" not in explicit["var0"] and "fss_useful_scale" not in explicit["var0"]
    assert torch.equal(explicit["var1"]["brier"], EV.brier_score(EV.event_counts(S, Tr, got, "below")[0].sum(dim=0)[1]))


# ------------------------------------------------------------------------------------------------------------------ argument errors

def test_argument_errors_are_value_errors(route):
    S, Tr = torch.zeros(2, 3, 2, 4, 8), torch.zeros(3, 2, 4, 8)
    thr = torch.zeros(2, 1)
    with pytest.raises(ValueError, match=r"samples \(2, 3, 2, 4, 8\) must be \(M >= 1,\) \+ truth \(3, 2, 4, 4\)"):
        EV.event_counts(S, Tr[..., :4], thr)
    with pytest.raises(ValueError, match="must be"):
        EV.fss_sums(S[:0], Tr, thr)
    with pytest.raises(ValueError, match="must be floating point"):
        EV.event_counts(S.long(), Tr, thr)
    for bad in (torch.zeros(3, 1), torch.zeros(2), torch.zeros(2, 0)):
        with pytest.raises(ValueError, match=r"thresholds .* must be \(F, K\)"):
            EV.event_counts(S, Tr, bad)
    with pytest.raises(ValueError, match="must be numbers"):
        EV.event_counts(S, Tr, torch.zeros(2, 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="must be 'above' or 'below'"):
        EV.event_counts(S, Tr, thr, "over")
    with pytest.raises(ValueError, match="direction must be"):
        EV.event_counts(S, Tr, thr, ["above", "below", "above"])
    for bad in ((), (-1,), (0, 1.5)):
        with pytest.raises(ValueError, match="radii .* must be at least one integer >= 0"):
            EV.fss_sums(S, Tr, thr, bad)
    sums = EV.fss_sums(S, Tr, thr, (1, 2))
    with pytest.raises(ValueError, match=r"radii \[1, 2\] must contain 0"):
        EV.member_contingency(sums, (1, 2), 32)
    with pytest.raises(ValueError, match="must contain 0"):
        EV.fss_useful_scale(sums, (1, 2), 32)
    with pytest.raises(ValueError, match="3 radii for sums"):
        EV.fss_useful_scale(sums, (0, 1, 2), 32)
    with pytest.raises(ValueError, match=r"sums .* must be \(T, F, K, S, M \+ 2, 2\)"):
        EV.fss(sums[0])
    with pytest.raises(ValueError, match=r"counts .* must be \(\.\.\., 2, M \+ 1\)"):
        EV.brier_score(torch.zeros(3, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"truth .* must be \(T, F, H, W\)"):
        EV.thresholds_from_quantiles(S)
    with pytest.raises(ValueError, match="1 names for 2 variables"):
        EV.events_report(S, Tr, thresholds=thr, names=["a"])
    with pytest.raises(ValueError, match=r"\(L, F, H, W\)"):
        EV.events_report(S, Tr[:2], thresholds=thr)
    g = torch.Generator().manual_seed(5)
    S2, T2 = torch.randn(2, 3, 2, 4, 8, generator=g), torch.randn(3, 2, 4, 8, generator=g)
    per_k = EV.event_counts(S2, T2, torch.zeros(2, 2), ["above", "below"])[0]  # one direction per threshold, for every variable
    assert torch.equal(per_k, EV.event_counts(S2, T2, torch.zeros(2, 2), [["above", "below"], ["above", "below"]])[0])
    assert torch.equal(per_k[:, :, 0], EV.event_counts(S2, T2, torch.zeros(2, 2), "above")[0][:, :, 0])
    assert not torch.equal(per_k[:, :, 1], EV.event_counts(S2, T2, torch.zeros(2, 2), "above")[0][:, :, 1])
    empty = EV.event_counts(S[:, :0], Tr[:0], thr)
    assert empty[0].shape == (0, 2, 1, 2, 3) and empty[1].shape == (0, 2) and EV.fss_sums(S[:, :0], Tr[:0], thr, (0,)).shape == (0, 2, 1, 1, 4, 2)


# ------------------------------------------------------------------------------------------------------------------ the host program

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_events(request, tmp_path_factory):
    """a stand-alone program, once plain and once under the address and undefined-behaviour sanitizers; it is run directly, never loaded
    into Python"""
    return host_program.build(tmp_path_factory, "events", sanitize=request.param == "sanitized", timeout=600)


@pytest.mark.parametrize("M,T,F,hw,K", [(1, 1, 1, 4, 1), (9, 2, 2, 4100, 3), (64, 1, 2, 4096, 8), (2, 1, 1, 16384, 2)])
def test_every_cell_is_binned_exactly_once_per_threshold(host_events, M, T, F, hw, K):
    """a plane smaller than a round, of one chunk, of a chunk + 4 cells and of four chunks; the bins of every plane add up to it"""
    rc = subprocess.run([str(host_events), "visit_counts"] + [str(a) for a in (M, T, F, hw, K)], timeout=600).returncode
    assert rc == 0, f"check {rc} of host_events_main.cpp failed"


@pytest.mark.parametrize("M,T,F,H,W_,K,radii", [(1, 1, 1, 4, 4, 1, (0,)), (2, 1, 2, 8, 12, 2, (0, 1, 2, 16)), (1, 1, 1, 64, 64, 1, (0, 16)),
                                               (2, 2, 1, 68, 72, 1, (0, 5, 16)), (1, 1, 1, 40, 132, 1, (0, 7)),
                                               (1, 1, 1, 130, 128, 1, (0, 1, 2, 3, 4, 8, 9, 16))])
def test_every_tile_halo_and_window_corner_is_walked_as_often_as_it_should_be(host_events, M, T, F, H, W_, K, radii):
    """planes clipped on all four sides, exactly one tile, remainder tiles of width 4 and 8, three tiles across, a remainder row of 2;
    a halo that is no multiple of 4; every cell staged once per tile whose halo reaches it and summed once per row and radius, every
    corner of the table read as often as the windows clipped to the domain say, nothing outside the domain"""
    args = [str(a) for a in (M, T, F, H, W_, K, len(radii)) + tuple(radii)]
    rc = subprocess.run([str(host_events), "visit_fss"] + args, timeout=600).returncode
    assert rc == 0, f"check {rc} of host_events_main.cpp failed"


def test_the_host_program_equals_the_reference(host_events, tmp_path):
    """csrc/events_core.h compiled for the host, every kind: the chunks, the derived bin, the tiles, the scans and the corner reads"""
    M, T, F, K = 3, 2, 2, 3
    for i, kind in enumerate(R.KINDS):
        H, W_ = ((41, 100), (68, 72), (8, 12))[i % 3]
        radii = ((0, 1, 16), (0, 3), (0, 1, 2, 4, 8, 16))[i % 3]
        x, y = R.fields(kind, M, T, F, H * W_)
        thr, above = R.thresholds(kind, y, K), R.directions(F, K, "mixed")
        files = [str(tmp_path / n) for n in ("x.f32", "y.f32", "thr.f32", "dir.i32", "a.i64", "b.i64")]
        for a, p in zip((x, y, thr, above.astype(np.int32)), files):
            a.tofile(p)
        rc = subprocess.run([str(host_events), "counts"] + [str(a) for a in (M, T, F, H * W_, K)] + files, timeout=600).returncode
        assert rc == 0
        want, winv = R.counts_ref(x, y, thr, above)
        assert np.array_equal(np.fromfile(files[4], np.int64).reshape(want.shape), want) and np.array_equal(np.fromfile(files[5], np.int64).reshape(winv.shape), winv)
        rc = subprocess.run([str(host_events), "fss"] + [str(a) for a in (M, T, F, H, W_, K, len(radii)) + radii] + files[:5], timeout=600).returncode
        assert rc == 0
        want = R.fss_ref(x, y, thr, above, radii, H, W_)
        assert np.array_equal(np.fromfile(files[4], np.int64).reshape(want.shape), want), kind


def test_the_emulation_restates_the_constants_of_the_kernel():
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "events_core.h")).read()
    for text in ("THREADS = 256", "MAX_M = 64, MAX_K = 8, MAX_S = 8, MAX_R = 16", "CHUNK = 4096", "TILE = 64", "REGION = TILE + 2 * MAX_R",
                 "static_assert(FSS_LDS_BYTES <= 160 * 1024", "hw >= 4 && hw % 4 == 0 && M >= 1 && M <= MAX_M && K >= 1 && K <= MAX_K"):
        assert text in core, text
    assert (emu_event_ops.THREADS, emu_event_ops.CHUNK, emu_event_ops.TILE, emu_event_ops.REGION) == (256, 4096, 64, 96)
    assert [emu_event_ops.chunks(hw) for hw in (4, 4096, 4100, 16384)] == [1, 1, 2, 4]
    assert emu_event_ops.geo_of(68, 72, 16, 0) == (0, 0, 64, 64, 0, 0, 68, 72) and emu_event_ops.geo_of(68, 72, 16, 3) == (64, 64, 4, 8, 48, 48, 20, 24)
    assert emu_event_ops.geo_of(200, 200, 5, 5) == (64, 64, 64, 64, 59, 56, 74, 80)  # the halo in x is rounded up to a multiple of 4


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_event_counts_supported": "int", "c2w_event_counts": "int", "c2w_fss_supported": "int", "c2w_fss_sums": "int"}
    c_abi.assert_declared(names, "events.hip", event_ops, ("counts_supported", "event_counts", "fss_supported", "fss_sums"))
