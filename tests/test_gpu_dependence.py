"""The co-moment kernel on the MI355X (csrc/comoments.hip through dependence_ops and climate2weather_amd.dependence): the tables EQUAL to
the NumPy reference of tests/fp64_comoments_ref.py, bit for bit -- one thread adds a series' terms in hour order, so there is no
tolerance -- at the smallest shapes that can go wrong, for every field kind, for an accumulator fed in cuts and wherever the planes
lie in a launch; the sums within the bound csrc/comoments_maps.h derives, against rational arithmetic; ``merge`` within its bound;
the report on the device against the same call on CPU tensors; an unsupported shape on the general route; known answers."""
import itertools

import numpy as np
import pytest
import torch

import emu_comoment_ops as E
import fp64_comoments_ref as R
from climate2weather_amd import dependence_ops
from climate2weather_amd import dependence as DP

pytestmark = pytest.mark.gpu
U = E.UNROLL


def dev():
    return torch.device("cuda:0")


def _case(kind, M, T, F, hw, seed):
    x, y = R.field(kind, (M, T, F, hw), seed), R.field(kind, (T, F, hw), seed + 1)
    return x, y, torch.from_numpy(x).view(M, T, F, hw // 4, 4).to(dev()), torch.from_numpy(y).view(T, F, hw // 4, 4).to(dev())


def _state(t):
    D, F = t.pivot.shape[:2]
    return dict(n=t.n.cpu().numpy().reshape(D, -1), pivot=t.pivot.cpu().numpy().reshape(D, F, -1),
                truth_pivot=None if t.truth_pivot is None else t.truth_pivot.cpu().numpy().reshape(D, F, -1),
                sums=t.sums.cpu().numpy().reshape(D, t.sums.shape[1], -1), invalid=t.invalid.cpu().numpy())


def _same(want, t):
    got = _state(t)
    return t.sums.is_cuda and R.same_bits(want, got["n"], got["pivot"], got["truth_pivot"], got["sums"], got["invalid"])


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 8])
def test_the_tables_equal_the_reference_bit_for_bit(F):
    """hw: one thread's cells, a ragged second chunk, five chunks; one member and three; with and without a truth; T = 1, the unroll,
    one more, three rounds and two; every field kind in turn"""
    c = E.chunk_cells(F)
    assert dependence_ops.supported(4, F) and c == 256 * E.cells_per_thread(F)
    combos = itertools.product((4, c + 4, 4 * c + 4), (1, 3), (True, False), (1, U, U + 1, 3 * U + 2))
    for i, (hw, M, with_truth, T) in enumerate(combos):
        kind = R.KINDS[(i + F) % len(R.KINDS)]
        x, y, xt, yt = _case(kind, M, T, F, hw, i)
        want = R.comoments(x, y if with_truth else None)
        assert _same(want, DP.comoments(xt, yt if with_truth else None)), (kind, hw, M, with_truth, T)


@pytest.mark.parametrize("kind", R.KINDS)
def test_an_accumulator_fed_in_cuts_equals_one_call(kind):
    M, T, F, hw = 2, 7, 2, E.chunk_cells(2) + 4
    x, y, xt, yt = _case(kind, M, T, F, hw, 77)
    want = R.comoments(x, y)
    one = DP.DependenceAccumulator(M, F, hw // 4, 4, device=dev()).update(xt, yt)
    cut = DP.DependenceAccumulator(M, F, hw // 4, 4, device=dev())
    for a, b in ((0, 1), (1, 1), (1, 2), (2, 4), (4, 7)):
        cut.update(xt[:, a:b], yt[a:b])
    assert _same(want, one.tables()) and _same(want, cut.tables())
    assert torch.equal(one.sums.view(torch.int64), cut.sums.view(torch.int64)) and torch.equal(one.n, cut.n)


def test_the_same_planes_at_two_positions_of_a_larger_launch_give_the_same_bits():
    M, T, F, hw = 4, 9, 3, 1028   # five chunks of 256 cells
    x, y, xt, yt = _case("nan_hours", M, T, F, hw, 5)
    xt[3] = xt[0]                                   # member 3 repeats member 0: rows far apart
    t = DP.comoments(xt, yt)
    assert torch.equal(t.sums[1].view(torch.int64), t.sums[4].view(torch.int64)) and torch.equal(t.n[1], t.n[4])
    assert torch.equal(t.pivot[1].view(torch.int32), t.pivot[4].view(torch.int32)) and torch.equal(t.invalid[1], t.invalid[4])
    a, b = 256 // 4, 516 // 4                       # cells 256 .. 515 as a launch of their own: other chunks, other threads
    sub = DP.comoments(xt[..., a:b, :].contiguous(), yt[..., a:b, :].contiguous())
    assert torch.equal(sub.sums.view(torch.int64), t.sums[:, :, a:b].contiguous().view(torch.int64)) and torch.equal(sub.n, t.n[:, a:b])
    assert torch.equal(sub.pivot.view(torch.int32), t.pivot[:, :, a:b].contiguous().view(torch.int32))


def _cells(hw):
    """the cells held against the rational reference: all of a small plane; the first and last threads, the seam between the chunks
    and every 97th cell of a large one (the bits do not depend on the position, which the test above holds)"""
    return list(range(hw)) if hw <= 64 else sorted(set(range(4)) | set(range(510, 516)) | set(range(hw - 4, hw)) | set(range(0, hw, 97)))


def test_the_sums_lie_within_the_derived_bound():
    worst = 0.0
    for hw in (4, 2 * E.chunk_cells(2) + 4):
        for kind in ("pressure", "smooth", "denormal", "pressure_tight"):
            x, y, xt, yt = _case(kind, 1, 50, 2, hw, 21)
            worst = max(worst, R.check_bound(x, y, _state(DP.comoments(xt, yt)), _cells(hw)))
    print(f"worst fraction of the bound on the device: {worst:.4f}")


def test_merge_of_two_device_accumulators_lies_within_its_bound():
    M, T, F, hw, cut = 2, 12, 2, E.chunk_cells(2) + 4, 5
    worst = 0.0
    for kind in ("pressure", "smooth", "nan_hours", "late_start"):
        x, y, xt, yt = _case(kind, M, T, F, hw, 31)
        a = DP.DependenceAccumulator(M, F, hw // 4, 4, device=dev()).update(xt[:, :cut], yt[:cut])
        b = DP.DependenceAccumulator(M, F, hw // 4, 4, device=dev()).update(xt[:, cut:], yt[cut:])
        t = a.merge(b).tables()
        assert t.sums.is_cuda
        worst = max(worst, R.check_merge(x[:, :cut], y[:cut], x[:, cut:], y[cut:], _state(t), _cells(hw)))
        one = R.comoments(x, y)
        assert np.array_equal(one["n"], _state(t)["n"]) and np.array_equal(one["invalid"], _state(t)["invalid"])
    print(f"worst fraction of the merge bound on the device: {worst:.4f}")


def test_the_report_on_the_device_equals_the_report_on_cpu_tensors():
    M, T, F, H, W = 3, 48, 3, 8, 8
    x, y = R.field("smooth", (M, T, F, H * W), 1), R.field("smooth", (T, F, H * W), 2)
    xc, yc = torch.from_numpy(x).view(M, T, F, H, W), torch.from_numpy(y).view(T, F, H, W)
    a, b = DP.dependence_report(xc.to(dev()), yc.to(dev())), DP.dependence_report(xc, yc)
    ta, tb = DP.comoments(xc.to(dev()), yc.to(dev())), DP.comoments(xc, yc)
    assert torch.equal(ta.sums.cpu().view(torch.int64), tb.sums.view(torch.int64)) and torch.equal(ta.n.cpu(), tb.n) and torch.equal(ta.invalid.cpu(), tb.invalid)
    for (name, va), (_, vb) in zip(a, b):
        assert set(va) == set(vb)
        for key in va:
            p, q = va[key], vb[key]
            if not p.is_floating_point():
                assert p.is_cuda and torch.equal(p.cpu(), q), (name, key)
            else:
                scale = float(q[~torch.isnan(q)].abs().max()) if bool((~torch.isnan(q)).any()) else 0.0
                assert p.is_cuda and p.dtype == torch.float64 and torch.allclose(p.cpu(), q, rtol=1e-12, atol=1e-12 * scale, equal_nan=True), (name, key)
    assert a.as_dict().keys() == b.as_dict().keys()


def test_an_unsupported_shape_takes_the_general_route_and_gives_the_same_bits():
    assert not dependence_ops.supported(6, 2) and not dependence_ops.supported(8, 9)
    for F, H, W in ((2, 2, 3), (9, 2, 4)):
        x, y = R.field("nan_hours", (2, 7, F, H * W), 3), R.field("nan_hours", (7, F, H * W), 4)
        xt, yt = torch.from_numpy(x).view(2, 7, F, H, W).to(dev()), torch.from_numpy(y).view(7, F, H, W).to(dev())
        assert _same(R.comoments(x, y), DP.comoments(xt, yt)), F


def test_known_answers_on_the_device():
    rng = np.random.default_rng(0)
    u = rng.integers(-50, 50, (1, 30, 1, 8)).astype(np.float32)
    xt = torch.from_numpy(np.concatenate([u, -4.0 * u + 3.0], axis=2)).view(1, 30, 2, 2, 4).to(dev())
    corr = DP.correlation(DP.comoments(xt))[0]
    assert corr.is_cuda and float((corr[0, 1] + 1.0).abs().max()) <= 2.0 ** -52 and float((corr[0, 0] - 1.0).abs().max()) <= 2.0 ** -52
    _, _, _, yt = _case("nan_hours", 1, 30, 2, 8, 2)
    t = DP.comoments(yt[None].expand(3, -1, -1, -1, -1), yt)
    s = DP.truth_statistics(t)
    ok = t.n[1:, None].expand_as(s.mean_bias) >= 2
    assert float(s.mean_bias[ok].abs().max()) == 0.0 and float(s.centred_rmse[ok].abs().max()) == 0.0
    assert s.std_ratio[ok].unique().tolist() == [1.0] and s.correlation[ok].unique().tolist() == [1.0]
    const = torch.full((2, 10, 2, 1, 4), 2.5, device=dev())
    tc = DP.comoments(const, const[0])
    assert float(DP.covariance(tc).abs().max()) == 0.0 and bool(torch.isnan(DP.correlation(tc)).all())
