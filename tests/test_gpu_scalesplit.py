"""The block-moment kernel on the MI355X (csrc/blockmoments.hip through scale_ops and climate2weather_amd.scalesplit): the tables EQUAL to
the NumPy reference of tests/fp64_blockmoments_ref.py, bit for bit -- the order of the adds is the definition, so there is no tolerance
-- at the smallest shapes that can go wrong, for every field kind and wherever the planes lie in a launch; the sums within the bound
csrc/blockmoments_maps.h derives, against rational arithmetic; the report on the device against the same call on CPU tensors; an
unsupported shape on the general route; known answers."""
import itertools

import numpy as np
import pytest
import torch

import fp64_blockmoments_ref as R
from climate2weather_amd import scale_ops
from climate2weather_amd import scalesplit as SS

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4, 4),         # one item
          (4, 8, 516),       # 258 items: a ragged second workgroup
          (8, 8, 8),         # one block
          (8, 16, 24),       # several blocks
          (16, 16, 16),      # one block
          (16, 128, 128),    # exactly one workgroup a plane
          (32, 32, 32),      # one block
          (32, 64, 96)]      # several blocks


def dev():
    return torch.device("cuda:0")


def _case(kind, M, T, F, H, W, seed):
    x, y = R.field(kind, (M, T, F, H, W), seed), R.field(kind, (T, F, H, W), seed + 1)
    return x, y, torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())


def _same(want, t):
    return t.sums.is_cuda and t.n.is_cuda and t.pivot.is_cuda and R.same_bits(want, t.n.cpu().numpy(), t.pivot.cpu().numpy(), t.sums.cpu().numpy())


def _state(t):
    return dict(n=t.n.cpu().numpy(), pivot=t.pivot.cpu().numpy(), sums=t.sums.cpu().numpy(), s=t.s)


def _integers(shape, seed, low=-20, high=20):
    return np.random.default_rng(seed).integers(low, high, shape).astype(np.float32)


@pytest.mark.parametrize("s,H,W", SHAPES)
def test_the_tables_equal_the_reference_bit_for_bit(s, H, W):
    """one member and three, one time and two, one variable and two, with and without a truth; every field kind in turn"""
    assert scale_ops.supported(H, W, s)
    for i, (M, T, F, with_truth) in enumerate(itertools.product((1, 3), (1, 2), (1, 2), (True, False))):
        kind = R.KINDS[(i + s // 4) % len(R.KINDS)]
        x, y, xt, yt = _case(kind, M, T, F, H, W, i)
        want = R.block_moments(x, y if with_truth else None, s)
        assert _same(want, SS.block_moments(xt, yt if with_truth else None, s)), (kind, M, T, F, with_truth)


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_field_kind_at_two_block_sizes(kind):
    for s, H, W in ((4, 8, 516), (16, 32, 48)):
        x, y, xt, yt = _case(kind, 2, 2, 1, H, W, 77)
        assert _same(R.block_moments(x, y, s), SS.block_moments(xt, yt, s)), s


@pytest.mark.parametrize("s", [4, 16])
def test_the_same_plane_at_two_positions_of_a_larger_launch_gives_the_same_bits(s):
    M, T, F, H, W = 4, 3, 2, 32, 80     # 160 or 40 items a plane: the planes lie across the workgroups
    x, y, xt, yt = _case("nan_cells", M, T, F, H, W, 5)
    xt[3, 2, 1] = xt[0, 0, 0]          # the plane of member 0 again, far away in the launch ...
    yt[2, 1] = yt[0, 0]                # ... and its truth
    t = SS.block_moments(xt, yt, s)
    for a in (t.sums.view(torch.int64), t.n, t.pivot.view(torch.int32)):
        assert torch.equal(a[1, 0, 0], a[4, 2, 1]) and torch.equal(a[0, 0, 0], a[0, 2, 1])
    sub = SS.block_moments(xt[1:3, 1:].contiguous(), yt[1:].contiguous(), s)   # a sub-range of planes as a launch of its own
    for a, b in ((sub.sums.view(torch.int64), t.sums.view(torch.int64)), (sub.n, t.n), (sub.pivot.view(torch.int32), t.pivot.view(torch.int32))):
        assert torch.equal(a[1:], b[2:4, 1:]) and torch.equal(a[0], b[0, 1:])


def test_the_sums_lie_within_the_derived_bound():
    worst = 0.0
    for s, H, W in ((4, 8, 516), (8, 16, 24), (16, 128, 128), (32, 64, 96)):
        for kind in ("pressure", "pressure_tight", "smooth", "denormal", "huge", "neg_zero"):
            x, y, xt, yt = _case(kind, 1, 1, 1, H, W, 21 + s)
            st = _state(SS.block_moments(xt, yt, s))
            worst = max(worst, R.check_bound(x, y, st, R.chosen_blocks(st["n"].shape, 6 if s < 32 else 3, seed=s)))
    print(f"worst fraction of the bound on the device: {worst:.4f}")


def _close(p, q):
    """a float64 device tensor against the CPU route's: rtol 1e-12, and as much of the largest entry for those that cancel"""
    scale = float(q[~torch.isnan(q)].abs().max()) if bool((~torch.isnan(q)).any()) else 0.0
    return p.is_cuda and p.dtype == torch.float64 and torch.allclose(p.cpu(), q, rtol=1e-12, atol=1e-12 * scale, equal_nan=True)


def test_the_report_on_the_device_equals_the_report_on_cpu_tensors():
    M, L, F, H, W, s, t_step = 3, 7, 2, 32, 32, 8, 6
    x, y = R.field("nan_cells", (M, L, F, H, W), 1), R.field("smooth", (L, F, H, W), 2)
    xc, yc = torch.from_numpy(x), torch.from_numpy(y)
    obs = torch.nn.functional.avg_pool2d(yc[::t_step], s)
    a, b = SS.scales_report(xc.to(dev()), yc.to(dev()), observation=obs.to(dev())), SS.scales_report(xc, yc, observation=obs)
    ta, tb = SS.block_moments(xc.to(dev()), yc.to(dev()), s), SS.block_moments(xc, yc, s)
    assert torch.equal(ta.sums.cpu().view(torch.int64), tb.sums.view(torch.int64)) and torch.equal(ta.n.cpu(), tb.n)
    assert (a.s, a.t_step) == (b.s, b.t_step) == (8, 6)
    for (name, va), (_, vb) in zip(a, b):
        assert set(va) == set(vb)
        for key in va:
            p, q = va[key], vb[key]
            if not p.is_floating_point():
                assert p.is_cuda and torch.equal(p.cpu(), q), (name, key)
            else:
                assert _close(p, q), (name, key)
    assert a.as_dict().keys() == b.as_dict().keys()
    pa, pb = SS.scale_profile(xc.to(dev()), yc.to(dev())), SS.scale_profile(xc, yc)
    for p, q in zip(pa[1:], pb[1:]):
        assert _close(p, q)


def test_an_unsupported_shape_takes_the_general_route_and_gives_the_same_bits():
    assert not scale_ops.supported(8, 8, 2) and not scale_ops.supported(16, 20, 8)
    for s, H, W in ((2, 8, 8), (5, 10, 20), (64, 64, 64)):
        x, y, xt, yt = _case("nan_cells", 2, 2, 2, H, W, 3)
        assert _same(R.block_moments(x, y, s), SS.block_moments(xt, yt, s)), s
    with pytest.raises(ValueError, match="s = 8 must divide H = 16 and W = 20"):   # W = 20, s = 8 has no blocks on any route ...
        SS.block_moments(torch.zeros(1, 1, 1, 16, 20, device=dev()), None, 8)
    x, y, xt, yt = _case("nan_cells", 2, 2, 2, 16, 20, 4)                          # ... and s = 4 on the same field takes the kernel
    assert scale_ops.supported(16, 20, 4) and _same(R.block_moments(x, y, 4), SS.block_moments(xt, yt, 4))


def test_known_answers_on_the_device():
    s, H, W = 4, 16, 12
    y = _integers((2, 2, H, W), 2)
    yt = torch.from_numpy(y).to(dev())
    t = SS.block_moments(yt[None].expand(2, -1, -1, -1, -1), yt, s)            # members equal to the truth
    split, ratio, corr = SS.error_split(t), SS.variance_ratio(t), SS.detail_correlation(t)
    assert split.total.is_cuda and float(split.coarse.abs().max()) == 0.0 and float(split.detail.abs().max()) == 0.0
    assert ratio.per_time.unique().tolist() == [1.0] and corr.per_time.unique().tolist() == [1.0] and corr.pooled.unique().tolist() == [1.0]
    k = _integers((2, 2, H // s, W // s), 3, -5, 6)                             # the truth plus a constant per block
    x = (y + np.repeat(np.repeat(k, s, axis=-2), s, axis=-1))[None]
    t = SS.block_moments(torch.from_numpy(x).to(dev()), yt, s)
    split = SS.error_split(t)
    assert float(split.detail.abs().max()) == 0.0 and torch.equal(split.coarse[0].cpu(), torch.from_numpy((k.astype(np.float64) ** 2).mean(axis=(-1, -2))))
    flat = np.ascontiguousarray(np.repeat(np.repeat(k, s, axis=-2), s, axis=-1)[None])   # constant on every block
    t = SS.block_moments(torch.from_numpy(flat).to(dev()), yt, s)
    assert float(SS.variance_ratio(t).per_time.abs().max()) == 0.0
    # a sum and one true division by a device tensor: torch's mean, and its division by a host scalar, multiply by a rounded 1 / 12
    blocks = torch.full((), float((H // s) * (W // s)), dtype=torch.float64, device=dev())
    assert torch.equal(SS.error_split(t).detail[0], SS.subgrid_variance(t)[0].sum(dim=(-1, -2)) / blocks)
    obs = SS.coarse(t)[0, ::2]                                                  # the truth row reproduces its own observation
    res = SS.observation_residual(t, obs, 2)
    assert res.rmse.is_cuda and float(res.bias[0].abs().max()) == 0.0 and float(res.rmse[0].abs().max()) == 0.0 and float(res.max_abs[0].abs().max()) == 0.0
