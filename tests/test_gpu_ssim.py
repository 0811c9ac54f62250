"""The SSIM kernel on the MI355X (csrc/ssim.hip through ops.ssim and ssim.ssim): every field kind, shape, window and batch shape
against the float64 definition by the rule of tests/fp64_ssim_ref.py -- a score passes if its error is at most four times the larger of
the fp32 pivoted avg_pool2d route's error on the same pair and 16 * 2^-24 -- then the properties the interface promises: the same bits
wherever a pair lies in the batch and whatever n_truth is, nothing written past n_pairs, nothing written for an unsupported shape, a NaN
kept in its own pair."""
import numpy as np
import pytest
import torch

import fp64_ssim_ref as R
from climate2weather_amd import ops
from climate2weather_amd import ssim as ssim_mod

pytestmark = pytest.mark.gpu

CANARY = -7.25


def dev():
    return torch.device("cuda:0")


def launch(x, y, rng, win, n_pairs=None, rows=None):
    """out (rows,) float64 from ops.ssim on the first n_pairs of x against all of y, rows past them holding the canary"""
    n, (H, W) = x.shape[0], x.shape[-2:]
    n_pairs = n if n_pairs is None else n_pairs
    out = torch.full((rows or n,), CANARY, dtype=torch.float64, device=x.device)
    assert ops.ssim(x, y, rng, out, n_pairs, y.shape[0], H, W, win)
    return out


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


@pytest.mark.parametrize("H,W,win,keep", [(16, 16, 7, 8), (16, 16, 11, 8), (16, 16, 15, 8), (24, 40, 15, 8), (32, 32, 15, 8), (64, 64, 15, 8),
                                          (128, 128, 15, 2), (128, 16, 7, 8), (40, 128, 11, 8)])
def test_every_field_kind_against_float64(H, W, win, keep):
    """one pair per kind, each with its own truth field and range (n_truth = n_pairs); at 128 x 128 the two pairs with offsets"""
    kinds, x, y, rng, S64, b = R.cases(H, W, win)
    sel = list(range(len(kinds))) if keep == 8 else [kinds.index("temperature"), kinds.index("pressure")]
    S = launch(*to_dev(x[sel], y[sel], rng[sel]), win).cpu().numpy()
    e = np.abs(S - S64[sel])
    print(f"{H}x{W} win {win}: error over max(yardstick, floor), limit {R.FACTOR}: " +
          ", ".join(f"{kinds[i]} {e[j] / (b[i] / R.FACTOR):.3g}" for j, i in enumerate(sel)))
    assert np.all(e <= b[sel]), [(kinds[i], e[j], b[i]) for j, i in enumerate(sel) if not e[j] <= b[i]]
    if keep == 8:
        assert abs(S[kinds.index("identical")] - 1.0) <= R.FACTOR * R.FLOOR and S[kinds.index("anti")] < 0


@pytest.mark.parametrize("H,W,win", [(16, 24, 7), (64, 48, 15)])
@pytest.mark.parametrize("n_pairs", [1, 3, 17])
def test_batch_shapes_pairing_and_per_slot_ranges(H, W, win, n_pairs):
    """n_pairs in {1, 3, 17} (none fills the last workgroup of four at W = 24) against n_truth in {1, 2, n_pairs}, ranges that differ by
    slot: pair i meets y[i % n_truth] and data_range[i % n_truth]"""
    g = np.random.default_rng(100 * n_pairs + H)
    for n_truth in sorted({1, min(2, n_pairs), n_pairs}):
        y = g.standard_normal((n_truth, H, W)).astype(np.float32)
        x = (y[np.arange(n_pairs) % n_truth] + 0.5 * g.standard_normal((n_pairs, H, W))).astype(np.float32)
        rng = (4.0 + 3.0 * np.arange(n_truth)).astype(np.float32)
        S = launch(*to_dev(x, y, rng), win).cpu().numpy()
        for i in range(n_pairs):
            t = i % n_truth
            S64 = R.ssim64(x[i], y[t], float(rng[t]), win)
            assert abs(S[i] - S64) <= R.bound(x[i], y[t], float(rng[t]), win, S64), (n_truth, i)
        if n_truth > 1:  # the ranges matter: the same pair under the other slot's range scores differently
            assert abs(R.ssim64(x[0], y[0], float(rng[1]), win) - R.ssim64(x[0], y[0], float(rng[0]), win)) > 1e-4


@pytest.mark.parametrize("H,W,win,n,rows", [(16, 16, 15, 5, 12), (32, 24, 7, 2, 9), (64, 64, 11, 2, 4), (128, 128, 15, 1, 3)])
def test_rows_past_n_pairs_keep_their_canary(H, W, win, n, rows):
    x = torch.randn(rows, H, W, device=dev())  # pairs past n_pairs exist and must not be read into a result either
    y = torch.randn(2, H, W, device=dev())
    out = launch(x, y, torch.full((2,), 6.0, device=dev()), win, n_pairs=n, rows=rows)
    assert torch.isfinite(out[:n]).all() and (out[:n].abs() <= 1.0 + 1e-6).all()
    assert torch.equal(out[n:], torch.full_like(out[n:], CANARY))


@pytest.mark.parametrize("H,W,win", [(16, 16, 15), (24, 32, 7), (64, 64, 15), (128, 128, 15)])
def test_same_bits_at_every_position_and_under_every_n_truth(H, W, win):
    """one pair at three positions of a batch of 11 (three different slots of a shared workgroup at W <= 32), under n_truth = 11 and
    n_truth = 1, alone, and on a second call"""
    g = np.random.default_rng(H + W)
    n, spots = 11, (0, 5, 10)
    px, py = R.pairs(H, W)["temperature"]
    x = (280.0 + 10.0 * g.standard_normal((n, H, W))).astype(np.float32)
    y = (280.0 + 10.0 * g.standard_normal((n, H, W))).astype(np.float32)
    for s in spots:
        x[s], y[s] = px, py
    rng = np.full(n, 77.0, dtype=np.float32)
    xd, yd, rd = to_dev(x, y, rng)
    a, b = launch(xd, yd, rd, win), launch(xd, yd, rd, win)
    assert torch.equal(a, b)
    alone = launch(*to_dev(px[None], py[None], rng[:1]), win)
    x1 = np.repeat(px[None], n, axis=0)
    one_truth = launch(*to_dev(x1, py[None], rng[:1]), win)  # n_truth = 1
    for s in spots:
        assert a[s].item() == alone[0].item(), s
    assert torch.equal(one_truth, alone[0].expand(n))


def test_nan_pair_gives_nan_and_spares_its_neighbours():
    for H, W in ((16, 16), (64, 64)):
        x, y = torch.randn(9, H, W, device=dev()), torch.randn(3, H, W, device=dev())
        x[4, 3, 3] = float("nan")
        out = launch(x, y, torch.full((3,), 6.0, device=dev()), 7)
        assert torch.isnan(out[4]) and torch.isfinite(out[:4]).all() and torch.isfinite(out[5:]).all()
        y[2, H - 1, W - 1] = float("nan")  # truth slot 2 meets pairs 2, 5, 8
        out = launch(x, y, torch.full((3,), 6.0, device=dev()), 7)
        assert torch.isnan(out[[2, 4, 5, 8]]).all() and torch.isfinite(out[[0, 1, 3, 6, 7]]).all()


@pytest.mark.parametrize("H,W,win", [(20, 20, 15), (256, 256, 15), (32, 32, 9)])
def test_unsupported_shapes_answer_false_write_nothing_and_take_the_general_route(H, W, win):
    assert not ops.ssim_supported(H, W, win)
    p = R.pairs(H, W)
    x, y = np.stack([p["smooth"][0], p["pressure"][0]]), np.stack([p["smooth"][1], p["pressure"][1]])
    rng = np.array([R.pair_range(x[i], y[i]) for i in range(2)], dtype=np.float32)
    xd, yd, rd = to_dev(x, y, rng)
    out = torch.full((2,), CANARY, dtype=torch.float64, device=dev())
    assert ops.ssim(xd, yd, rd, out, 2, 2, H, W, win) is False
    assert torch.equal(out, torch.full_like(out, CANARY))
    S = ssim_mod.ssim(xd, yd, data_range=rd, win_size=win)
    assert S.is_cuda and S.dtype == torch.float64
    for i in range(2):
        S64 = R.ssim64(x[i], y[i], float(rng[i]), win)
        assert abs(S[i].item() - S64) <= R.bound(x[i], y[i], float(rng[i]), win, S64)


def test_kernel_and_general_route_agree_on_a_strided_half_precision_input():
    base = torch.randn(2, 3, 32, 64, device=dev()).to(torch.float16)
    view, truth = base[..., ::2], base[0, :, :, 1::2]  # (2, 3, 32, 32) against (3, 32, 32)
    got = ssim_mod.ssim(view, truth, data_range=8.0, win_size=15)
    assert got.shape == (2, 3) and got.dtype == torch.float64 and got.is_cuda
    x, y = view.float().contiguous(), truth.float().contiguous()
    general = torch.empty(6, dtype=torch.float64, device=dev())
    ssim_mod._ssim_general(x.view(6, 32, 32), y, torch.full((3,), 8.0, device=dev()), general, 15)
    xn, yn = x.cpu().numpy(), y.cpu().numpy()
    for m in range(2):
        for f in range(3):
            S64 = R.ssim64(xn[m, f], yn[f], 8.0, 15)
            b = R.bound(xn[m, f], yn[f], 8.0, 15, S64)
            assert abs(got[m, f].item() - S64) <= b and abs(general[3 * m + f].item() - S64) <= b


def test_report_on_the_device_equals_the_cpu_report():
    """(M, T, F) = (2, 3, 2) at 24 x 40, de-normalised (temperature-like and pressure-like): the device report (kernel) against the
    CPU report (float64 general route), each score by the rule; the mean over time of scores within b is within b"""
    g = np.random.default_rng(9)
    off, sd = np.array([280.0, 101325.0]), np.array([10.0, 1200.0])
    truth = np.stack([np.stack([off[f] + sd[f] * R.smooth(24, 40, 70 + 10 * t + f) for f in range(2)]) for t in range(3)]).astype(np.float32)
    samples = (truth[None] + 0.3 * sd[None, None, :, None, None] * g.standard_normal((2, 3, 2, 24, 40))).astype(np.float32)
    cpu = ssim_mod.ssim_report(torch.tensor(samples), torch.tensor(truth), names=["tas", "psl"])
    gpu = ssim_mod.ssim_report(*to_dev(samples, truth), names=["tas", "psl"])
    for f, (name, v) in enumerate(gpu):
        assert v["ssim_over_time"].is_cuda and v["ssim_over_time"].shape == (2, 3) and v["ssim"].shape == (2,)
        R_f = float(cpu[name]["data_range"])
        assert float(v["data_range"]) == R_f
        want = cpu[name]["ssim_over_time"].numpy()
        b = np.array([[R.bound(samples[m, t, f], truth[t, f], R_f, 15, want[m, t]) for t in range(3)] for m in range(2)])
        e = np.abs(v["ssim_over_time"].cpu().numpy() - want)
        print(f"{name}: error over max(yardstick, floor) {np.max(e / (b / R.FACTOR)):.3g}")
        assert np.all(e <= b)
        assert np.all(np.abs(v["ssim"].cpu().numpy() - cpu[name]["ssim"].numpy()) <= b.max(axis=1))
    assert set(gpu.as_dict()) == set(cpu.as_dict())
