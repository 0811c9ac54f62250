"""The marginals kernels on the MI355X (csrc/kde.hip through ops.kde_eval, ops.pit_counts and climate2weather_amd.marginals): every
density entry against float64 by the rule of tests/fp64_kde_ref.py -- an entry passes if its error is at most four times the larger of
the pivoted fp32 torch route's error on that entry and the floor of 16 * 2^-24 relative in u -- the rank histogram against the
reference's line of numpy bit for bit, then the properties the interface promises: the same bits wherever a data set lies in the launch,
nothing written past the end, nothing written for an unsupported shape, a NaN kept in its own row."""
import numpy as np
import pytest
import torch

import fp64_kde_ref as R
from climate2weather_amd import marginals as Mg
from climate2weather_amd import ops

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 64  # canary values behind each output


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


def kde(x, y, g, h, expect=True):
    """dens (D, N) float64 from ops.kde_eval on x (n_rep, T, F, hw), y (T, F, hw) or None, the float64 grid g (F, N) and the
    bandwidths h (D,); the TAIL values behind dens and behind the scratch must keep the canary.  expect False: the call must answer
    False and leave every value of both buffers alone."""
    n_rep, T, F, hw = x.shape
    N = g.shape[1]
    D = n_rep * F + (F if y is not None else 0)
    piv = [R.pivot_and_offsets(g[f]) for f in range(F)]
    xd, offd, pivd, hd = to_dev(x, np.stack([p[1] for p in piv]), np.array([p[0] for p in piv], np.float32), np.asarray(h, np.float64))
    yd = None if y is None else to_dev(y)[0]
    nd = max(1, ops.kde_scratch_bytes(D, T * hw, N) // 8) if expect else 4096
    scratch = torch.full((nd + TAIL,), CANARY, dtype=torch.float64, device=dev())
    dens = torch.full((D * N + TAIL,), CANARY, dtype=torch.float64, device=dev())
    ok = ops.kde_eval(xd, yd, offd, pivd, hd, scratch[:nd], dens, n_rep, T, F, hw, N)
    assert ok is expect
    keep_from = D * N if expect else 0
    assert torch.equal(dens[keep_from:], torch.full_like(dens[keep_from:], CANARY))
    assert torch.equal(scratch[nd if expect else 0:], torch.full_like(scratch[nd if expect else 0:], CANARY))
    return dens[:D * N].view(D, N)


def pit(samples, truth, expect=True):
    """counts (F, M + 1) int64 from ops.pit_counts; the TAIL values behind it must keep the canary"""
    M, T, F = samples.shape[:3]
    hw = int(np.prod(samples.shape[3:]))
    n = F * (M + 1)
    buf = torch.full((n + TAIL,), -7, dtype=torch.int64, device=dev())
    sd, td = to_dev(samples, truth)
    assert ops.pit_counts(sd, td, buf, M, T, F, hw) is expect
    keep_from = n if expect else 0
    assert torch.equal(buf[keep_from:], torch.full_like(buf[keep_from:], -7))
    return buf[:n].view(F, M + 1).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ density

SHAPES = [(1, 1, 1, 64), (2, 3, 2, 64), (3, 5, 4, 192), (1, 2, 1, 1024)]
GRIDS = [1, 7, 256, 1000, 1024]


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("n_rep,T,F,hw", SHAPES)
def test_density_entries_against_float64(n_rep, T, F, hw, N):
    """every field kind, samples and truth in one launch; variable f differs from its neighbours in pivot, h and grid, so a wrong
    i % F fails"""
    worst = {}
    for kind in R.KINDS:
        s, t, g, h, f64, b = R.reference(kind, n_rep, T, F, hw, N)
        got = kde(s, t, g, h).cpu().numpy()
        worst[kind], ok = R.worst(got, f64, b)
        assert ok, (kind, worst[kind])
    print(f"(n_rep, T, F, hw) {(n_rep, T, F, hw)} N {N}: error over max(yardstick, floor), limit {R.FACTOR}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_density_over_several_chunks_and_folds():
    """n = 13 x 256 = 3328: three chunks of 1024 and a fourth of 256 (one 256-term chain; the full ones hold four), two variables"""
    worst = {}
    for kind in R.KINDS:
        s, t, g, h, f64, b = R.reference(kind, 1, 13, 2, 256, 1000)
        worst[kind], ok = R.worst(kde(s, t, g, h).cpu().numpy(), f64, b)
        assert ok, (kind, worst[kind])
    print(f"n 3328 (4 chunks) N 1000: error over max(yardstick, floor), limit {R.FACTOR}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_density_same_bits_at_every_position():
    """one data set first, in the middle and last among the samples, as the truth, alone, and on a second call"""
    T, hw, N = 13, 256, 1000
    s, t = R.fields("temperature", 3, T, 2, hw)
    s, t = s.copy(), t.copy()
    s[1, :, 1] = s[2, :, 1] = t[:, 0] = s[0, :, 0]  # data sets 0, 3, 5 of the samples and 6, the truth's first
    g = np.repeat(R.grid64(s, t, N)[:1], 2, axis=0)  # one grid for both variables
    h = R.bandwidths(s, t)
    assert h[0] == h[3] == h[5] == h[6]
    a, b = kde(s, t, g, h), kde(s, t, g, h)
    assert torch.equal(a, b)
    alone = kde(s[:1, :, :1], None, g[:1], h[:1])
    for ds in (0, 3, 5, 6):
        assert torch.equal(a[ds], alone[0]), ds
    assert not torch.equal(a[1], alone[0])
    as_truth = kde(s[1:2], s[0], g, np.concatenate([h[2:4], h[0:2]]))  # the same values where the truth rides
    assert torch.equal(as_truth[2], alone[0])


def test_density_unsupported_shapes_write_nothing_and_take_the_general_route():
    assert not ops.kde_supported(66, 16) and not ops.kde_supported(64, 1025) and not ops.kde_supported(64, 0)
    assert ops.kde_supported(4, 1) and ops.kde_supported(16384, 1024)
    for hw, N in ((66, 16), (64, 1025)):
        s, t = R.fields("wind", 2, 3, 2, hw)
        g, h = R.grid64(s, t, N), R.bandwidths(s, t)
        kde(s, t, g, h, expect=False)
        H, W_ = (6, 11) if hw == 66 else (8, 8)
        got, got_t = Mg.gaussian_kde(*to_dev(s.reshape(2, 3, 2, H, W_)), *to_dev(g), truth=to_dev(t.reshape(3, 2, H, W_))[0])
        assert got.is_cuda and got.shape == (2, 2, N) and got_t.shape == (2, N)
        rows = [R.bound(v, g[f], h[i]) for i, (f, v) in enumerate(R.data_sets(s, t))]
        ratio, ok = R.worst(torch.cat([got.reshape(-1, N), got_t]).cpu().numpy(), np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
        assert ok, (hw, N, ratio)


def test_density_nan_stays_in_its_row():
    s, t = R.fields("white", 3, 4, 2, 256)
    g = R.grid64(s, t, 300)
    S, Tr, G = to_dev(s.reshape(3, 4, 2, 16, 16), t.reshape(4, 2, 16, 16), g)
    clean, clean_t = Mg.gaussian_kde(S, G, truth=Tr)
    S[1, 2, 0, 3, 3] = float("nan")
    S[2, 3, 1, 15, 15] = float("inf")
    Tr[0, 1, 0, 0] = float("nan")
    got, got_t = Mg.gaussian_kde(S, G, truth=Tr)
    bad = torch.zeros(3, 2, dtype=torch.bool, device=dev())
    bad[1, 0] = bad[2, 1] = True
    assert torch.equal(torch.isnan(got).all(dim=-1), bad) and torch.equal(torch.isnan(got).any(dim=-1), bad)
    assert torch.isnan(got_t[1]).all() and torch.equal(got_t[0], clean_t[0]) and torch.equal(got[~bad], clean[~bad])
    # the kernel's own detection, with a finite bandwidth handed in
    s2 = s.copy()
    s2[0, 1, 1, 7] = np.inf
    d = kde(s2, t, g, R.bandwidths(s, t)).cpu().numpy()
    assert np.isnan(d[1]).all() and not np.isnan(np.delete(d, 1, axis=0)).any()


def test_strided_half_precision_input_agrees_with_the_dense_route():
    base = (torch.randn(2, 5, 3, 16, 32, device=dev()) * 3.0 + 1.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]
    g = torch.linspace(-12.0, 14.0, 200, dtype=torch.float64, device=dev())[None].expand(3, 200)
    got, got_t = Mg.gaussian_kde(view, g, truth=truth)
    dense, dense_t = Mg.gaussian_kde(view.float().contiguous(), g, truth=truth.float().contiguous())
    assert got.shape == (2, 3, 200) and torch.equal(got, dense) and torch.equal(got_t, dense_t)


# ------------------------------------------------------------------------------------------------------------------ rank histogram

def _pit_case(M, T, F, H, W_, seed=0):
    g = np.random.default_rng(seed)
    truth = g.standard_normal((T, F, H, W_)).astype(np.float32)
    samples = (0.3 * np.arange(F)[None, None, :, None, None] + 1.2 * g.standard_normal((M, T, F, H, W_))).astype(np.float32)
    samples[0, 0, 0, 0, :2] = truth[0, 0, 0, :2]  # ties
    samples[M - 1, T - 1, F - 1, 1, 1] = np.nan
    truth[0, 0, 2, 3] = np.nan
    return samples, truth


@pytest.mark.parametrize("T,F,H,W_", [(3, 2, 8, 8), (2, 4, 16, 24), (1, 1, 8, 4)])
@pytest.mark.parametrize("M", [1, 2, 8, 33, 64])
def test_pit_counts_are_the_numpy_statement(M, T, F, H, W_):
    samples, truth = _pit_case(M, T, F, H, W_, M + T)
    got = pit(samples, truth)
    assert np.array_equal(got, R.pit64(samples, truth))
    assert np.array_equal(got.sum(-1), np.full(F, T * H * W_))
    again = Mg.pit_counts(*to_dev(samples, truth))
    assert again.is_cuda and again.dtype == torch.int64 and np.array_equal(again.cpu().numpy(), got)


def test_pit_exact_cases():
    M, T, F, H, W_ = 4, 2, 2, 4, 4
    cells = T * H * W_
    truth = np.zeros((T, F, H, W_), np.float32)
    above, below = np.ones((M, T, F, H, W_), np.float32), -np.ones((M, T, F, H, W_), np.float32)
    assert pit(above, truth).tolist() == [[cells, 0, 0, 0, 0]] * F   # truth below all members: all mass in bin 0
    assert pit(below, truth).tolist() == [[0, 0, 0, 0, cells]] * F   # truth above all members: all mass in bin M
    tie = above.copy()
    tie[2] = 0.0                                                      # a tie counts
    assert pit(tie, truth).tolist() == [[0, cells, 0, 0, 0]] * F
    nan_member = below.copy()
    nan_member[1, :, 1] = np.nan                                      # a NaN member is never <=
    assert pit(nan_member, truth).tolist() == [[0, 0, 0, 0, cells], [0, 0, 0, cells, 0]]
    nan_truth = truth.copy()
    nan_truth[0, 0] = np.nan                                          # a NaN truth gives bin 0
    assert pit(below, nan_truth).tolist() == [[H * W_, 0, 0, 0, cells - H * W_], [0, 0, 0, 0, cells]]
    assert pit(np.full((M, T, F, H, W_), -0.0, np.float32), truth).tolist() == [[0, 0, 0, 0, cells]] * F  # -0 <= +0


def test_pit_with_more_planes_than_workgroups():
    """2500 planes of one variable: the launcher caps the grid at eight workgroups a CU (2048 on 256 CUs), so some walk two planes;
    and three variables at 900 times each, where every workgroup keeps its variable"""
    for M, T, F, H, W_ in ((2, 2500, 1, 8, 4), (3, 900, 3, 4, 4)):
        samples, truth = _pit_case(M, T, F, H, W_, T)
        assert np.array_equal(pit(samples, truth), R.pit64(samples, truth))


def test_pit_unsupported_shapes_write_nothing_and_take_the_general_route():
    assert not ops.pit_supported(66, 8) and not ops.pit_supported(64, 65) and not ops.pit_supported(64, 0)
    assert ops.pit_supported(4, 1) and ops.pit_supported(16384, 64)
    for M, H, W_ in ((65, 8, 8), (4, 6, 11)):
        samples, truth = _pit_case(M, 3, 2, H, W_, M)
        pit(samples, truth, expect=False)
        got = Mg.pit_counts(*to_dev(samples, truth))
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), R.pit64(samples, truth))


# ------------------------------------------------------------------------------------------------------------------ the report

def test_report_on_the_device_equals_the_cpu_report():
    """(M, T, F) = (2, 5, 2) at 16 x 24, de-normalised (temperature-like and pressure-like), 100 points: the grid and the counts
    exactly; the densities by the rule, with the CPU report -- the float64 formula -- as the float64 side"""
    rng = np.random.default_rng(9)
    off, sd = np.array([280.0, 101325.0]), np.array([10.0, 1200.0])
    truth = (off[None, :, None, None] + sd[None, :, None, None] * rng.standard_normal((5, 2, 16, 24))).astype(np.float32)
    samples = (off[None, None, :, None, None] + 1.3 * sd[None, None, :, None, None] * rng.standard_normal((2, 5, 2, 16, 24))).astype(np.float32)
    cpu = Mg.marginals_report(torch.tensor(samples), torch.tensor(truth), n_points=100, names=["tas", "psl"])
    gpu = Mg.marginals_report(*to_dev(samples, truth), n_points=100, names=["tas", "psl"])
    for f, (name, v) in enumerate(gpu):
        c = cpu[name]
        assert all(t.is_cuda for t in v.values())
        assert torch.equal(v["x"].cpu(), c["x"]) and torch.equal(v["counts"].cpu(), c["counts"]) and torch.equal(v["density"].cpu(), c["density"])
        x = c["x"].numpy()
        sets = [(truth[:, f].reshape(-1), v["gt"], c["gt"])] + [(samples[m, :, f].reshape(-1), v["samples"][m], c["samples"][m]) for m in range(2)]
        for vals, got, want in sets:
            h = vals.size ** -0.2 * np.std(vals.astype(np.float64), ddof=1)
            f64, floor = R.kde64(vals, x, h)
            assert np.allclose(want.numpy(), f64, rtol=1e-11, atol=0)  # the CPU report is the formula
            _, b = R.bound(vals, x, h, f64, floor)
            ratio, ok = R.worst(got.cpu().numpy(), want.numpy(), b)
            print(f"{name}: device against CPU report: error over max(yardstick, floor) {ratio:.3g} (limit {R.FACTOR})")
            assert ok
    assert torch.equal(gpu.all_variables["counts"].cpu(), cpu.all_variables["counts"])
    assert set(gpu.as_dict()) == set(cpu.as_dict())
