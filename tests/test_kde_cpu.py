"""CPU checks of the ensemble marginals (climate2weather_amd.marginals): both routes of gaussian_kde -- the general float64 one and the
launcher's, with tests/emu_kde_ops.py standing in for the HIP kernels -- against the float64 definition by the rule of
tests/fp64_kde_ref.py, the definition itself against scipy.stats.gaussian_kde, the report against a line-by-line restatement of the
reference's figure code, the exact cases of the rank histogram, the rule's negative control, the argument checks, the kernels' own index
maps and arithmetic compiled for the host (csrc/kde_core.h) under the address and undefined-behaviour sanitizers, and the C declarations
against the ctypes prototypes."""
import os
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_kde_ops
import fp64_kde_ref as R
import host_program
from climate2weather_amd import marginals as Mg
from climate2weather_amd import ops as c2w_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of marginals.gaussian_kde and marginals.pit_counts on CPU tensors"""
    if request.param == "launcher":
        emu_kde_ops.install(monkeypatch, c2w_ops, Mg)
    return request.param


def _t5(s, t, H, W_):
    """(n_rep, T, F, hw), (T, F, hw) arrays -> the (n_rep, T, F, H, W), (T, F, H, W) tensors of the public interface"""
    return torch.tensor(s).view(s.shape[:3] + (H, W_)), torch.tensor(t).view(t.shape[:2] + (H, W_))


# ------------------------------------------------------------------------------------------------------------------ both routes

@pytest.mark.parametrize("n_rep,T,F,H,W_,N", [(2, 3, 2, 8, 8, 1000), (1, 5, 1, 25, 40, 1000), (3, 2, 4, 4, 6, 7)])
def test_every_field_kind_against_float64(route, n_rep, T, F, H, W_, N):
    """n = 192, 5000 (five chunks of the launcher's, the last one partly filled) and 48"""
    for kind in R.KINDS:
        s, t, g, h, f64, b = R.reference(kind, n_rep, T, F, H * W_, N)
        S, Tr = _t5(s, t, H, W_)
        got, got_t = Mg.gaussian_kde(S, torch.tensor(g), truth=Tr)
        assert got.dtype == torch.float64 and got.shape == (n_rep, F, N) and got_t.shape == (F, N)
        hh = torch.cat([Mg.bandwidth(S).reshape(-1), Mg.bandwidth(Tr)]).numpy()
        assert np.allclose(hh, h, rtol=1e-12, atol=0)
        ratio, ok = R.worst(np.concatenate([got.numpy().reshape(-1, N), got_t.numpy()]), f64, b)
        print(f"{route} {kind} {(n_rep, T, F, H * W_, N)}: error over max(yardstick, floor) {ratio:.3g} (limit {R.FACTOR})")
        assert ok, kind
        alone = Mg.gaussian_kde(S, torch.tensor(g))  # without the truth: the same rows
        assert torch.equal(alone, got)


def test_any_dtype_any_strides_and_leading_dimensions(route):
    base = 280.0 + 10.0 * torch.randn(2, 3, 4, 2, 8, 16, dtype=torch.float64)
    view = base[..., ::2]  # (2, 3, 4, 2, 8, 8), strided
    for cast in (torch.float64, torch.float16):
        v32 = view.to(cast).float().numpy().reshape(6, 4, 2, 64)
        g = R.grid64(v32, v32[0], 33)
        got = Mg.gaussian_kde(view.to(cast), torch.tensor(g), bw_method="silverman")
        assert got.shape == (2, 3, 2, 33) and got.dtype == torch.float64
        h = R.bandwidths(v32, None, "silverman")
        for i, (f, v) in enumerate(R.data_sets(v32)):
            f64, b = R.bound(v, g[f], h[i])
            assert R.worst(got.numpy().reshape(6, 2, 33)[i // 2, i % 2], f64, b)[1], (cast, i)


@pytest.mark.parametrize("bw_method", ["scott", "silverman", 0.37])
def test_the_definition_is_scipy_s(route, bw_method):
    """scipy.stats.gaussian_kde with its defaults, as exp/figures.py:64 calls it, on pressure-like values"""
    stats = pytest.importorskip("scipy.stats")
    n = 5000
    s, t = R.fields("pressure", 1, 5, 1, 1000)
    v = s[0, :, 0].reshape(-1)
    g = np.linspace(v.min(), v.max(), 200)
    want = stats.gaussian_kde(v.astype(np.float64), bw_method=bw_method)(g)
    h = R.factor(n, bw_method) * np.std(v.astype(np.float64), ddof=1)
    f64, floor = R.kde64(v, g, h)
    rel = np.max(np.abs(f64 - want) / want)
    print(f"{bw_method}: the float64 formula against scipy.stats.gaussian_kde, n = {n}: max relative difference {rel:.3g}")
    assert rel <= 1e-12
    got = Mg.gaussian_kde(torch.tensor(s).view(1, 5, 1, 25, 40), torch.tensor(g)[None], bw_method=bw_method)
    _, b = R.bound(v, g, h, f64, floor)
    assert np.all(np.abs(got.numpy()[0, 0] - want) <= b + 1e-12 * want)


def test_a_nan_or_inf_value_poisons_its_own_row_only(route):
    s, t = R.fields("temperature", 3, 4, 2, 64)
    g = R.grid64(s, t, 50)
    S, Tr = _t5(s, t, 8, 8)
    S, Tr = S.clone(), Tr.clone()
    S[1, 2, 0, 3, 3] = float("nan")
    S[2, 0, 1, 0, 0] = float("inf")
    Tr[3, 1, 7, 7] = float("-inf")
    got, got_t = Mg.gaussian_kde(S, torch.tensor(g), truth=Tr)
    bad = torch.zeros(3, 2, dtype=torch.bool)
    bad[1, 0] = bad[2, 1] = True
    assert torch.equal(torch.isnan(got).all(dim=-1), bad) and torch.equal(torch.isnan(got).any(dim=-1), bad)
    assert torch.equal(torch.isnan(got_t).all(dim=-1), torch.tensor([False, True])) and not torch.isnan(got_t[0]).any()
    clean = Mg.gaussian_kde(torch.tensor(s).view(3, 4, 2, 8, 8), torch.tensor(g))
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1, 1], clean[1, 1])


def test_degenerate_data_sets_are_nan_where_scipy_raises(route):
    g = torch.linspace(0.0, 6.0, 5, dtype=torch.float64)[None]
    assert torch.isnan(Mg.gaussian_kde(torch.full((2, 1, 2, 4), 3.0), g)).all()  # zero spread: h = 0
    assert torch.isnan(Mg.gaussian_kde(torch.full((1, 1, 1, 1), 3.0), g)).all()  # n = 1
    assert torch.isnan(Mg.bandwidth(torch.rand(1, 1, 1, 1))).all()  # n = 1: std with ddof = 1 is 0 / 0


# ------------------------------------------------------------------------------------------------------------------ the rank histogram

def _pit_case(M, T, F, H, W_, seed=0):
    g = np.random.default_rng(seed)
    truth = g.standard_normal((T, F, H, W_)).astype(np.float32)
    samples = (0.3 * np.arange(F)[None, None, :, None, None] + 1.2 * g.standard_normal((M, T, F, H, W_))).astype(np.float32)
    samples[0, 0, 0, 0, :2] = truth[0, 0, 0, :2]  # ties
    return samples, truth


@pytest.mark.parametrize("M,T,F,H,W_", [(1, 3, 2, 8, 8), (8, 2, 4, 16, 24), (33, 1, 1, 8, 4), (64, 3, 2, 2, 6), (3, 5, 2, 5, 5)])
def test_pit_counts_are_the_reference_s_line(route, M, T, F, H, W_):
    samples, truth = _pit_case(M, T, F, H, W_, M)
    got = Mg.pit_counts(torch.tensor(samples), torch.tensor(truth))
    assert got.dtype == torch.int64 and got.shape == (F, M + 1)
    assert np.array_equal(got.numpy(), R.pit64(samples, truth))
    assert np.array_equal(got.sum(-1).numpy(), np.full(F, T * H * W_))


def test_pit_exact_cases(route):
    M, T, F, H, W_ = 4, 2, 2, 4, 4
    cells = T * H * W_
    truth = torch.zeros(T, F, H, W_)
    above, below = torch.ones(M, T, F, H, W_), -torch.ones(M, T, F, H, W_)
    assert Mg.pit_counts(above, truth).tolist() == [[cells, 0, 0, 0, 0]] * F   # truth below all members: all mass in bin 0
    assert Mg.pit_counts(below, truth).tolist() == [[0, 0, 0, 0, cells]] * F   # truth above all members: all mass in bin M
    tie = above.clone()
    tie[2] = 0.0                                                                # a tie counts
    assert Mg.pit_counts(tie, truth).tolist() == [[0, cells, 0, 0, 0]] * F
    nan_member = below.clone()
    nan_member[1, :, 1] = float("nan")                                          # a NaN member is never <=
    assert Mg.pit_counts(nan_member, truth).tolist() == [[0, 0, 0, 0, cells], [0, 0, 0, cells, 0]]
    nan_truth = truth.clone()
    nan_truth[0, 0] = float("nan")                                              # a NaN truth gives bin 0
    assert Mg.pit_counts(below, nan_truth).tolist() == [[H * W_, 0, 0, 0, cells - H * W_], [0, 0, 0, 0, cells]]
    neg_zero = torch.full((M, T, F, H, W_), -0.0)
    assert Mg.pit_counts(neg_zero, truth).tolist() == [[0, 0, 0, 0, cells]] * F   # -0 <= +0


# ------------------------------------------------------------------------------------------------------------------ report

def _ensemble(H, W_, M=3, T=5, seed=5):
    """de-normalised: variable 0 temperature-like, variable 1 pressure-like"""
    rng = np.random.default_rng(seed)
    off, sd = np.array([280.0, 101325.0]), np.array([10.0, 1200.0])
    truth = off[None, :, None, None] + sd[None, :, None, None] * rng.standard_normal((T, 2, H, W_))
    samples = off[None, None, :, None, None] + 1.2 * sd[None, None, :, None, None] * rng.standard_normal((M, T, 2, H, W_))
    return samples.astype(np.float32), truth.astype(np.float32)


def _trapezoid(y, x):
    return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(x)))


def _reference_figure(samples, truth, N):
    """exp/figures.py:52-86 line by line, with the float64 formula in gaussian_kde's place (verified against it above)"""
    num_samples, F = samples.shape[0], truth.shape[1]
    kde_x = np.stack([np.linspace(min(truth[:, i].min().item(), samples[:, :, i].min().item()),
                                  max(truth[:, i].max().item(), samples[:, :, i].max().item()), N) for i in range(F)])

    def gaussian_kde(values):
        values = values.astype(np.float64)
        h = values.size ** -0.2 * np.std(values, ddof=1)
        return lambda x: R.kde64(values, x, h)[0]

    kde_gt = np.stack([gaussian_kde(truth[:, i].reshape(-1))(kde_x[i]) for i in range(F)])
    kde_samples = np.stack([np.stack([gaussian_kde(samples[s, :, i].reshape(-1))(kde_x[i]) for i in range(F)]) for s in range(num_samples)])
    return kde_x, kde_gt, kde_samples


@pytest.mark.parametrize("H,W_,N", [(8, 8, 1000), (16, 24, 100)])
def test_report_against_the_reference_figure(route, H, W_, N):
    samples, truth = _ensemble(H, W_)
    M, T = samples.shape[0], samples.shape[1]
    rep = Mg.marginals_report(torch.tensor(samples), torch.tensor(truth), n_points=N, names=["tas", "psl"])
    kde_x, kde_gt, kde_samples = _reference_figure(samples, truth, N)
    hist, hist_all = R.pit_histogram_reference(samples, truth)
    counts = R.pit64(samples, truth)
    assert rep.names == ["tas", "psl"]
    for f, (name, v) in enumerate(rep):
        assert set(v) == {"x", "gt", "samples", "counts", "density"} and rep[name] is v
        assert np.array_equal(v["x"].numpy(), kde_x[f])  # numpy.linspace bit for bit
        assert v["gt"].shape == (N,) and v["samples"].shape == (M, N) and v["gt"].dtype == torch.float64
        sets = [truth[:, f].reshape(-1)] + [samples[m, :, f].reshape(-1) for m in range(M)]
        got = [v["gt"].numpy()] + [v["samples"][m].numpy() for m in range(M)]
        want = [kde_gt[f]] + [kde_samples[m, f] for m in range(M)]
        for vals, a, w in zip(sets, got, want):
            h = vals.size ** -0.2 * np.std(vals.astype(np.float64), ddof=1)
            _, b = R.bound(vals, kde_x[f], h, w, R.kde64(vals, kde_x[f], h)[1])
            ratio, ok = R.worst(a, w, b)
            assert ok, (name, ratio)
        assert np.array_equal(v["counts"].numpy(), counts[f]) and int(v["counts"].sum()) == T * H * W_
        assert np.allclose(v["density"].numpy(), hist[f], rtol=1e-12, atol=0)
    assert np.array_equal(rep.all_variables["counts"].numpy(), counts.sum(axis=0))
    assert np.allclose(rep.all_variables["density"].numpy(), hist_all, rtol=1e-12, atol=0)
    flat = rep.as_dict()
    assert set(flat) == {f"marginals/{n}/{k}" for n in ("tas", "psl") for k in ("pit_mean", "pit_outside", "kde_l1")} | {
        "marginals/all_variables/pit_mean", "marginals/all_variables/pit_outside"}
    assert all(isinstance(x, float) for x in flat.values())
    c = counts[1].astype(np.float64)
    assert flat["marginals/psl/pit_mean"] == pytest.approx((c * np.arange(M + 1)).sum() / (M * c.sum()), rel=1e-12)
    assert flat["marginals/psl/pit_outside"] == pytest.approx((c[0] + c[M]) / c.sum(), rel=1e-12)
    assert flat["marginals/tas/kde_l1"] == pytest.approx(np.mean([_trapezoid(np.abs(kde_samples[m, 0] - kde_gt[0]), kde_x[0]) for m in range(M)]), rel=1e-6)


def test_report_names_and_argument_checks(route):
    samples, truth = _ensemble(8, 8)
    S, Tr = torch.tensor(samples), torch.tensor(truth)
    rep = Mg.marginals_report(S, Tr, n_points=1)
    assert rep.names == ["var0", "var1"] and rep["var0"]["x"].shape == (1,) and set(rep.as_dict("eval")) >= {"eval/var1/kde_l1"}
    assert float(rep["var1"]["x"][0]) == min(truth[:, 1].min(), samples[:, :, 1].min())
    with pytest.raises(ValueError):
        Mg.marginals_report(S, Tr[:2])
    with pytest.raises(ValueError):
        Mg.marginals_report(S, Tr, names=["only_one"])
    with pytest.raises(ValueError):
        Mg.marginals_report(S, Tr, n_points=0)
    with pytest.raises(ValueError):
        Mg.marginals_report(S[0], Tr)


def test_argument_checks():
    x, g = torch.zeros(2, 3, 2, 8, 8), torch.zeros(2, 5, dtype=torch.float64)
    with pytest.raises(ValueError):
        Mg.gaussian_kde(x[0, 0], g)
    with pytest.raises(ValueError):
        Mg.gaussian_kde(x, g[:1])
    with pytest.raises(ValueError):
        Mg.gaussian_kde(x, g[:, :0])
    with pytest.raises(ValueError):
        Mg.gaussian_kde(x, g[0])
    with pytest.raises(ValueError):
        Mg.gaussian_kde(x, g, truth=torch.zeros(3, 2, 8, 4))
    with pytest.raises(ValueError):
        Mg.gaussian_kde(x, g, bw_method="epanechnikov")
    with pytest.raises(ValueError):
        Mg.gaussian_kde(x[:, :0], g)
    with pytest.raises(ValueError):
        Mg.bandwidth(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError):
        Mg.pit_counts(x, torch.zeros(3, 2, 8, 4))
    with pytest.raises(ValueError):
        Mg.pit_counts(x[:0], x[0])
    empty = Mg.gaussian_kde(torch.zeros(0, 3, 2, 8, 8), g)
    assert empty.shape == (0, 2, 5) and empty.dtype == torch.float64


def test_unsupported_shapes_take_the_general_route(monkeypatch):
    """hw no multiple of 4, N > 1024 and M > 64: the launcher is asked, answers no, nothing is launched, the general route answers"""
    emu_kde_ops.install(monkeypatch, c2w_ops, Mg)
    for H, W_, N in ((5, 5, 16), (8, 8, 1025)):
        s, t, g, h, f64, b = R.reference("wind", 2, 3, 2, H * W_, N)
        S, Tr = _t5(s, t, H, W_)
        got, got_t = Mg.gaussian_kde(S, torch.tensor(g), truth=Tr)
        assert emu_kde_ops.CALLS == []
        assert R.worst(np.concatenate([got.numpy().reshape(-1, N), got_t.numpy()]), f64, b)[1]
    samples, truth = _pit_case(65, 2, 1, 8, 8)
    assert np.array_equal(Mg.pit_counts(torch.tensor(samples), torch.tensor(truth)).numpy(), R.pit64(samples, truth))
    odd_s, odd_t = _pit_case(3, 2, 1, 5, 5)
    assert np.array_equal(Mg.pit_counts(torch.tensor(odd_s), torch.tensor(odd_t)).numpy(), R.pit64(odd_s, odd_t))
    assert emu_kde_ops.CALLS == [("pit", 65, 2, 1, 64), ("pit", 3, 2, 1, 25)]  # the launcher was asked, answered no and wrote nothing
    s, t = R.fields("white", 2, 3, 2, 64)
    Mg.marginals_report(*_t5(s, t, 8, 8), n_points=9)
    assert emu_kde_ops.CALLS[-2:] == [("kde", 2, 3, 2, 64, 9, True), ("pit", 2, 3, 2, 64)]  # samples and truth in ONE launch


# ------------------------------------------------------------------------------------------------------------------ the rule bites

NEGATIVE_N = 50000  # see the first test below
_NEG = {}


def _negative_case():
    """pressure-like values of one data set, n = NEGATIVE_N, 250 grid points: (samples, values, grid, h, f64, floor), computed once"""
    if not _NEG:
        s, t = R.fields("pressure", 1, 50, 1, NEGATIVE_N // 50)
        v = s[0, :, 0].reshape(-1)
        g = R.grid64(s, t, 250)[0]
        h = R.factor(NEGATIVE_N) * np.std(v.astype(np.float64), ddof=1)
        _NEG["case"] = (s, v, g, h) + R.kde64(v, g, h)
    return _NEG["case"]


def test_the_straight_fp32_port_fails_the_rule_on_pressure_like_fields():
    """the float64 grid rounded to fp32 and g - x on the raw values, no pivot: a grid point near 1e5 moves by up to 2^-8 = 0.0039, which
    is that over h in u.  h shrinks as n^(-1/5), so n was raised on the CPU until the port fails clearly: n = 50000 was taken (the
    printed line says by how much)."""
    s, v, g, h, f64, floor = _negative_case()
    _, b = R.bound(v, g, h, f64, floor)
    e_naive = np.abs(R.naive32(v, g, h) - f64)
    print(f"pressure-like, n = {NEGATIVE_N}, h = {h:.4g}: straight fp32 port, error / bound (limit 1): median {np.median(e_naive / b):.3g} max "
          f"{np.max(e_naive / b):.3g}, entries over the bound {int((e_naive > b).sum())} of {b.size}")
    assert not np.all(e_naive <= b) and np.max(e_naive / b) > 1.5  # the rule asks every entry to pass


def test_the_kernel_s_arithmetic_passes_where_the_straight_port_fails(monkeypatch):
    emu_kde_ops.install(monkeypatch, c2w_ops, Mg)
    s, v, g, h, f64, floor = _negative_case()
    got = Mg.gaussian_kde(torch.tensor(s).view(1, 50, 1, 25, 40), torch.tensor(g)[None]).numpy()[0, 0]
    e = np.abs(got - f64)
    print(f"pressure-like, n = {NEGATIVE_N}: the kernel's arithmetic (emulated), error over the floor alone: max {np.max(e / floor):.3g}")
    assert np.all(e <= R.FACTOR * floor)  # the rule with the floor alone


# ------------------------------------------------------------------------------------------------------------------ the kernels' maps

@pytest.fixture(scope="module")
def host_kde(tmp_path_factory):
    """a stand-alone program under the address and undefined-behaviour sanitizers; it is run directly, never loaded into Python"""
    return host_program.build(tmp_path_factory, "kde", sanitize=True, timeout=300)


@pytest.mark.parametrize("n_rep,T,F,hw,N", [(2, 3, 2, 100, 1000), (1, 13, 1, 256, 300), (3, 1, 4, 4, 1), (1, 7, 3, 36, 1024)])
def test_every_value_and_grid_point_is_visited_exactly_once(host_kde, tmp_path, n_rep, T, F, hw, N):
    """n = 300, 3328 (three chunks and a quarter), 4, 252: none a multiple of the chunk; N = 1000, 300 and 1 are no multiple of the 256
    threads.  The fields hold their own indices, so what was fetched says where from."""
    subprocess.run([str(host_kde), "visit", str(n_rep), str(T), str(F), str(hw), str(N), str(tmp_path / "ox.i32"), str(tmp_path / "oy.i32")],
                   check=True, timeout=300)
    ox, oy = np.fromfile(tmp_path / "ox.i32", dtype=np.int32), np.fromfile(tmp_path / "oy.i32", dtype=np.int32)
    want_x = np.broadcast_to((np.arange(n_rep)[:, None, None, None] * F + np.arange(F)[None, None, :, None]), (n_rep, T, F, hw))
    want_y = np.broadcast_to(n_rep * F + np.arange(F)[None, :, None], (T, F, hw))
    assert np.array_equal(ox.reshape(n_rep, T, F, hw), want_x) and np.array_equal(oy.reshape(T, F, hw), want_y)


@pytest.mark.parametrize("n_rep,T,F,hw,N", [(2, 3, 2, 64, 1000), (1, 13, 1, 256, 300), (2, 2, 3, 20, 7)])
def test_density_phases_on_the_host_meet_the_rule(host_kde, tmp_path, n_rep, T, F, hw, N):
    """csrc/kde_core.h compiled for the host: the chunk bounds, the value map, the point map, the 256-term fold and the fold over the
    chunks, every kind by the rule; a NaN value gives its row NaN and no other"""
    for kind in R.KINDS:
        s, t, g, h, f64, b = R.reference(kind, n_rep, T, F, hw, N)
        s = s.copy()
        if kind == "white":
            s[0, T - 1, F - 1, hw - 1] = np.nan
        piv = [R.pivot_and_offsets(g[f]) for f in range(F)]
        for name, a, dt in (("x", s, np.float32), ("y", t, np.float32), ("off", np.stack([p[1] for p in piv]), np.float32),
                            ("piv", np.array([p[0] for p in piv]), np.float32), ("h", h, np.float64)):
            np.ascontiguousarray(a, dtype=dt).tofile(tmp_path / name)
        subprocess.run([str(host_kde), "density", str(n_rep), str(T), str(F), str(hw), str(N), "1"] +
                       [str(tmp_path / n) for n in ("x", "y", "off", "piv", "h", "dens")], check=True, timeout=300)
        got = np.fromfile(tmp_path / "dens", dtype=np.float64).reshape(-1, N)
        keep = np.ones(got.shape[0], bool)
        if kind == "white":
            keep[F - 1] = False
            assert np.isnan(got[F - 1]).all()
        ratio, ok = R.worst(got[keep], f64[keep], b[keep])
        print(f"{kind} {(n_rep, T, F, hw, N)}: error over max(yardstick, floor) {ratio:.3g} (limit {R.FACTOR})")
        assert ok and not np.isnan(got[keep]).any(), kind


@pytest.mark.parametrize("M,T,F,hw,grid", [(1, 3, 2, 64, 6), (8, 7, 2, 384, 4), (64, 2, 1, 4, 1), (33, 5, 3, 2048, 6)])
def test_rank_histogram_phases_on_the_host(host_kde, tmp_path, M, T, F, hw, grid):
    """one workgroup per plane, workgroups that walk several times (7 times over 2 per variable), a plane of one quad, and a plane of
    two quads per thread; ties and NaNs on both sides"""
    samples, truth = _pit_case(M, T, F, hw // 4, 4, M + T)
    samples[M - 1, T - 1, F - 1, 0, 1] = np.nan
    truth[0, 0, 0, 3] = np.nan
    samples.tofile(tmp_path / "x"), truth.tofile(tmp_path / "y")
    subprocess.run([str(host_kde), "pit", str(M), str(T), str(F), str(hw), str(grid), str(tmp_path / "x"), str(tmp_path / "y"), str(tmp_path / "c")],
                   check=True, timeout=300)
    assert np.array_equal(np.fromfile(tmp_path / "c", dtype=np.int64).reshape(F, M + 1), R.pit64(samples, truth))


def test_support_predicates_and_chunking_agree():
    for hw, N, want in ((4, 1, True), (16384, 1024, True), (66, 16, False), (0, 16, False), (64, 1025, False), (64, 0, False)):
        assert emu_kde_ops.kde_supported(hw, N) is want
    for hw, M, want in ((4, 1, True), (16384, 64, True), (66, 8, False), (64, 65, False), (64, 0, False)):
        assert emu_kde_ops.pit_supported(hw, M) is want
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "kde_core.h")).read()
    for text in ("THREADS = 256", "MAX_N = 1024", "TILE = 4 * THREADS", "FOLD = 256", "MAX_CHUNKS = 64", "PIT_MAX_M = 64", "PIT_COPIES = 16",
                 "hw % 4 == 0 && N >= 1 && N <= MAX_N", "hw % 4 == 0 && M >= 1 && M <= PIT_MAX_M"):
        assert text in core, text
    # the chunk length depends on n alone: one tile up to 65536 values, 64 chunks beyond; the reference's own shape
    assert [emu_kde_ops.chunk_len(n) for n in (1, 1024, 1025, 65536, 65537, 1457 * 16384)] == [1024, 1024, 1024, 1024, 2048, 373760]
    assert [emu_kde_ops.chunks(n) for n in (1, 1024, 1025, 3328, 65536, 65537, 1457 * 16384)] == [1, 1, 2, 4, 64, 33, 64]
    assert emu_kde_ops.kde_scratch_bytes(36, 1457 * 16384, 1000) == 36 * 64 * 1000 * 8


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_kde_supported": "int", "c2w_kde_scratch_bytes": "long long", "c2w_kde_eval": "int", "c2w_kde_partial": "int", "c2w_kde_fold": "int", "c2w_pit_supported": "int",
             "c2w_pit_counts": "int"}
    c_abi.assert_declared(names, "kde.hip")
