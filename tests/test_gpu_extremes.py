"""The extremes kernels on the MI355X (csrc/extremes.hip through extreme_ops and climate2weather_amd.extremes): the block extremes
EQUAL to the NumPy reference of tests/fp64_extremes_ref.py, bit for bit -- integer compares on keys carry no tolerance -- at the
smallest shapes that can go wrong, for every field kind, for an accumulator fed in cuts and wherever the planes lie in a launch; the
L-moments within the bound csrc/extremes_maps.h derives, against rational arithmetic; the device's bits next to those of the NumPy
restatement of the host compile (printed, and asserted equal: the first run showed equality); the report on the device against the
same call on CPU tensors; an unsupported shape on the general route."""
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

import emu_extreme_ops
import fp64_extremes_ref as R
from climate2weather_amd import extreme_ops
from climate2weather_amd import extremes as EX

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().cpu().view(torch.int32).numpy().view(np.uint32)


def _case(kind, M, T, F, hw, seed, block):
    x, y = R.field(kind, (M, T, F, hw), seed, block), R.field(kind, (T, F, hw), seed + 1, block)
    return x, y, torch.from_numpy(x).view(M, T, F, hw // 4, 4).to(dev()), torch.from_numpy(y).view(T, F, hw // 4, 4).to(dev())


def test_the_block_extremes_equal_the_reference_bit_for_bit():
    """hw: one thread's cells, a ragged second chunk, five chunks; one member and three; with and without a truth; block 1, 3, 24
    against T = 1, 7, 50 (blocks that end with the call, inside it, never); every field kind in turn, mixed directions"""
    F, dirs = 2, ["max", "min"]
    combos = itertools.product((4, 1028, 4100), (1, 3), (True, False), (1, 3, 24), (1, 7, 50))
    for i, (hw, M, with_truth, block, T) in enumerate(combos):
        kind = R.KINDS[i % len(R.KINDS)]
        x, y, xt, yt = _case(kind, M, T, F, hw, i, block)
        for partial in ("drop", "keep"):
            want, invalid = R.block_extremes_by_planes(x, y if with_truth else None, block, [True, False], partial == "keep")
            t = EX.block_extremes(xt, yt if with_truth else None, block, dirs, partial)
            what = (kind, hw, M, with_truth, block, T, partial)
            assert t.n_blocks == want.shape[2] and np.array_equal(_bits(t.extremes).reshape(want.shape), want), what
            assert np.array_equal(t.invalid.cpu().numpy(), invalid), what


@pytest.mark.parametrize("kind", R.KINDS)
def test_an_accumulator_fed_in_cuts_equals_one_call(kind):
    M, T, F, hw, block = 2, 7, 2, 1028, 3
    x, y, xt, yt = _case(kind, M, T, F, hw, 77, block)
    want, invalid = R.block_extremes_by_planes(x, y, block, [False, True], True)
    one = EX.ExtremeAccumulator(M, F, hw // 4, 4, block, ["min", "max"], max_blocks=2, device=dev()).update(xt, yt)
    cut = EX.ExtremeAccumulator(M, F, hw // 4, 4, block, ["min", "max"], max_blocks=2, device=dev())
    for a, b in ((0, 1), (1, 2), (2, 4), (4, 7)):
        cut.update(xt[:, a:b], yt[a:b])
    for acc in (one, cut):
        t = acc.tables("keep")
        assert np.array_equal(_bits(t.extremes).reshape(want.shape), want) and np.array_equal(t.invalid.cpu().numpy(), invalid)
        assert t.open_hours == 1 and acc.tables().n_blocks == 2
    assert torch.equal(one.open, cut.open) and torch.equal(one.table.view(torch.int32), cut.table.view(torch.int32))


def test_the_same_planes_at_two_positions_of_a_larger_launch_give_the_same_bits():
    M, T, F, hw, block = 4, 9, 3, 2052, 4
    x, y, xt, yt = _case("nan_hours", M, T, F, hw, 5, block)
    xt[3], xt[:, :, 2], yt[:, 2] = xt[0], xt[:, :, 0], yt[:, 0]   # member 3 repeats member 0, variable 2 repeats variable 0: rows far apart
    t = EX.block_extremes(xt, yt, block, "max", "keep")
    b = t.extremes.view(torch.int32)
    assert torch.equal(b[1], b[4]) and torch.equal(b[:, 0], b[:, 2]) and torch.equal(t.invalid[:, 0], t.invalid[:, 2])
    lm, nv = EX.lmoments(t.extremes)
    assert torch.equal(lm[1].view(torch.int64), lm[4].view(torch.int64)) and torch.equal(lm[:, 0].view(torch.int64), lm[:, 2].view(torch.int64))
    half = EX.lmoments(t.extremes[1:2, :1, :, 256:])[0]  # the same cells as another row at another offset of another launch
    assert torch.equal(half.view(torch.int64), lm[1:2, :1, :, 256:].contiguous().view(torch.int64))


def _cells(hw):
    """the cells held against the rational reference: all of a small plane; the first and last threads, the seam between the chunks
    and every 41st cell of a large one (the bits do not depend on the position, which the test above holds)"""
    return list(range(hw)) if hw <= 64 else sorted(set(range(8)) | set(range(1016, hw)) | set(range(0, hw, 41)))


@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 16, 17, 33, 64])
def test_the_lmoments_lie_within_the_derived_bound(n):
    for hw in (4, 1028):
        Rr = 3
        t = np.concatenate([R.field("pressure", (1, n, 1, hw), n).reshape(1, n, hw), R.field("smooth", (1, n, 1, hw), n + 1).reshape(1, n, hw),
                            R.field("denormal", (1, n, 1, hw), n + 2).reshape(1, n, hw)])
        t[1] = np.where(np.random.default_rng(n).random((n, hw)) < 0.3, np.float32(np.nan), t[1])   # NaN extremes: n' varies from cell to cell
        lm, nv = EX.lmoments(torch.from_numpy(t).view(Rr, n, hw // 4, 4).to(dev()))
        lm, nv = lm.cpu().numpy().reshape(Rr, 4, hw), nv.cpu().numpy().reshape(Rr, hw)
        cells = _cells(hw)
        worst = R.check_lmoments(t[:, :, cells], lm[:, :, cells], nv[:, cells])
        host_lm, host_nv = torch.empty((Rr, 4, hw), dtype=torch.float64), torch.empty((Rr, hw), dtype=torch.int32)
        assert emu_extreme_ops.lmoments(torch.from_numpy(t), host_lm, host_nv, Rr, n, hw)     # tests/test_extremes_cpu.py: the host compile's bits
        same = np.array_equal(host_lm.numpy(), lm, equal_nan=True)
        print(f"n = {n}, hw = {hw}: worst fraction of the bound {worst:.3f}; device bits equal to the host's: {same}")
        assert np.array_equal(host_nv.numpy(), nv)
        assert same


def test_the_report_on_the_device_equals_the_report_on_cpu_tensors():
    M, T, F, H, W, block = 3, 48, 2, 8, 8, 6
    x, y = R.field("smooth", (M, T, F, H * W), 1), R.field("smooth", (T, F, H * W), 2)
    xc, yc = torch.from_numpy(x).view(M, T, F, H, W), torch.from_numpy(y).view(T, F, H, W)
    args = (block, ["max", "min"], [2, 5, 20])
    a, b = EX.extremes_report(xc.to(dev()), yc.to(dev()), *args), EX.extremes_report(xc, yc, *args)
    ta, tb = EX.block_extremes(xc.to(dev()), yc.to(dev()), block, args[1]), EX.block_extremes(xc, yc, block, args[1])
    assert torch.equal(ta.extremes.cpu().view(torch.int32), tb.extremes.view(torch.int32)) and torch.equal(ta.invalid.cpu(), tb.invalid)
    for (name, va), (_, vb) in zip(a, b):
        assert set(va) == set(vb)
        for key in va:
            p, q = va[key], vb[key]
            if not torch.is_tensor(p):
                assert p == q, key
            elif not p.is_floating_point():
                assert p.is_cuda and torch.equal(p.cpu(), q), (name, key)
            else:
                scale = float(q[~torch.isnan(q)].abs().max()) if bool((~torch.isnan(q)).any()) else 0.0
                assert p.is_cuda and p.dtype == torch.float64 and torch.allclose(p.cpu(), q, rtol=1e-12, atol=1e-12 * scale, equal_nan=True), (name, key)
    assert a.as_dict().keys() == b.as_dict().keys()


def test_an_unsupported_shape_takes_the_general_route_and_gives_the_same_answer():
    assert not extreme_ops.update_supported(6, 3, 2) and not extreme_ops.lmoments_supported(6, 2) and not extreme_ops.lmoments_supported(8, 65)
    x, y = R.field("nan_hours", (2, 7, 2, 6), 3), R.field("nan_hours", (7, 2, 6), 4)
    xt, yt = torch.from_numpy(x).view(2, 7, 2, 2, 3).to(dev()), torch.from_numpy(y).view(7, 2, 2, 3).to(dev())
    want, invalid = R.block_extremes(x, y, 3, [True, False], True)
    t = EX.block_extremes(xt, yt, 3, ["max", "min"], "keep")
    assert np.array_equal(_bits(t.extremes).reshape(want.shape), want) and np.array_equal(t.invalid.cpu().numpy(), invalid)
    lm, nv = EX.lmoments(t.extremes)
    cpu_lm, cpu_nv = EX.lmoments(t.extremes.cpu())
    assert lm.is_cuda and torch.equal(nv.cpu(), cpu_nv) and torch.allclose(lm.cpu(), cpu_lm, rtol=1e-13, atol=0, equal_nan=True)
    R.check_lmoments(_bits(t.extremes).view(np.float32).reshape(6, 3, 6), lm.cpu().numpy().reshape(6, 4, 6), nv.cpu().numpy().reshape(6, 6))


def test_known_answers_on_the_device():
    n = 12
    t = torch.arange(n, dtype=torch.float32, device=dev()).flip(0).view(n, 1, 1).expand(n, 2, 4).contiguous()
    lm, nv = EX.lmoments(t)
    assert nv.unique().tolist() == [n] and lm[0].unique().tolist() == [(n - 1) / 2]
    A = sum(abs(Fraction(j - n // 2)) for j in range(n))
    for r, want in ((1, Fraction(n + 1, 6)), (2, Fraction(0)), (3, Fraction(0))):
        assert abs(Fraction(float(lm[r, 0, 0])) - want) <= R.lmoment_bound(r + 1, n, A, Fraction(n - 1, 2))
    _, _, xt, yt = _case("smooth", 1, 40, 2, 8, 9, 5)
    samples = yt[None].expand(3, -1, -1, -1, -1).contiguous()
    ext = EX.block_extremes(samples, yt, 5, "max").extremes
    lm, _ = EX.lmoments(ext)
    xi, alpha, k, unfitted = EX.gev_fit(lm)
    assert all(float(a.abs().max()) == 0.0 for a in EX.mean_extreme_error(lm) + EX.return_level_error(EX.gev_return_level(xi, alpha, k, [2, 10]))[:2])
    pit = EX.gev_pit(ext, xi, alpha, k)
    assert pit.is_cuda and pit.sum(dim=-1).tolist() == [[8 * int((~torch.isnan(xi[0, f])).sum()) for f in range(2)]] * 3
