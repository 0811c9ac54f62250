"""The noise stream of the training run (csrc/philox.h) against its independent float64 definition (tests/fp64_noise_ref.py), element by
element: c2w_philox_normal itself, the power of that comparison against planted defects, and the element index with which the kernels
that regenerate the stream (csrc/pointwise.hip) address it."""
import pytest
import torch

import fp64_noise_ref as N
import fp64_ref as R
from climate2weather_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = ops.DTYPE_F32, ops.DTYPE_BF16, ops.DTYPE_F16
TD = ops.TORCH_DTYPE
N_STREAM = 1_000_003  # not a multiple of 4: the tail of the last block
SEEDS = [0, 1, 1 << 32, 0xFFFFFFFF, 2 ** 64 - 1, 0x0123456789ABCDEF, 2 ** 62 - 1]
MIXED = 0x0123456789ABCDEF
# max |c2w_philox_normal - normal_stream| over N_STREAM elements, measured on an MI355X (float32 __logf, sqrtf, __sincosf and the float32
# angle against float64 on the same float32 u).  N.STREAM_ERR is the largest of them, N.STREAM_TOL = 4 x that is asserted below.
STREAM_ERR_BY_SEED = {
    0: 1.754982e-06,
    1: 1.665779e-06,
    1 << 32: 1.748076e-06,
    0xFFFFFFFF: 1.775381e-06,
    2 ** 64 - 1: 1.608147e-06,
    0x0123456789ABCDEF: 1.755506e-06,
    2 ** 62 - 1: 1.828193e-06,
}
_cache = {}


def _stream(seed, n=N_STREAM):
    """(kernel's stream as float64, reference) on the device, computed once per seed"""
    if (seed, n) not in _cache:
        out = torch.full((n + 5,), 7.0, device=DEV)
        ops.philox_normal(out, n, seed)
        assert (out[n:] == 7.0).all(), "c2w_philox_normal wrote past n"
        _cache[(seed, n)] = (out[:n].double(), torch.from_numpy(N.normal_stream(n, seed)).to(DEV))
    return _cache[(seed, n)]


def test_the_asserted_tolerance_is_four_times_the_measurement_and_under_the_cap():
    assert N.STREAM_ERR == max(STREAM_ERR_BY_SEED.values()) and set(STREAM_ERR_BY_SEED) == set(SEEDS)
    assert N.STREAM_TOL == 4 * N.STREAM_ERR and 0 < N.STREAM_TOL <= N.STREAM_TOL_CAP == 2.0 ** -11


@pytest.mark.parametrize("seed", SEEDS)
def test_philox_normal_against_the_float64_definition(seed):
    got, ref = _stream(seed)
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    print(f"stream vs float64 definition, seed {seed:#x}: max err {err.max().item():.3e} at element {int(err.argmax())}, "
          f"mean err {err.mean().item():.3e}, max |z| {ref.abs().max().item():.3f}")
    assert err.max().item() <= N.STREAM_TOL
    unit = torch.from_numpy(N.unit_u0_mask(N_STREAM, seed)).to(DEV)
    assert (got[unit] == 0).all()


def test_a_radius_of_exactly_zero():
    """seed 5947: u0 of block 41 rounds to 1.0 (tests/test_noise_ref_cpu.py): elements 164 and 165 are exactly 0, nothing is NaN"""
    n = 256
    got, ref = _stream(5947, n)
    unit = torch.from_numpy(N.unit_u0_mask(n, 5947)).to(DEV)
    assert int(unit.sum()) == 2 and torch.isfinite(got).all()
    assert (got[unit] == 0).all() and (got[~unit] != 0).all()
    assert (got - ref).abs().max().item() <= N.STREAM_TOL


DEFECTS = {
    "seed + 1": lambda n, s: N.normal_stream(n, s + 1),
    "seed ^ (1 << 32)": lambda n, s: N.normal_stream(n, s ^ (1 << 32)),
    "key words swapped": lambda n, s: N.normal_stream(n, s, swap_key=True),
    "counter one block ahead": lambda n, s: N.normal_stream(n, s, block_shift=1),
    "lanes 1 and 2 swapped": lambda n, s: N.normal_stream(n, s, lanes=(0, 2, 1, 3)),
    "cos and sin swapped": lambda n, s: N.normal_stream(n, s, swap_trig=True),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
@pytest.mark.parametrize("seed", [MIXED, 1])
def test_the_comparison_rejects_planted_defects(seed, defect):
    """The defect is planted in the reference: the kernel's stream must then violate the same tolerance on more than 90 % of the
    elements the defect touches -- all of them, except for the lane swap, which by construction leaves lanes 0 and 3 (half of the
    stream) where they were: there it is 90 % of lanes 1 and 2, and so more than 45 % of all elements."""
    got, ref = _stream(seed)
    assert ((got - ref).abs() > N.STREAM_TOL).sum().item() == 0
    bad = (got - torch.from_numpy(DEFECTS[defect](N_STREAM, seed)).to(DEV)).abs() > N.STREAM_TOL
    touched = torch.ones_like(bad)
    if defect == "lanes 1 and 2 swapped":
        lane = torch.arange(N_STREAM, device=DEV) & 3
        touched = (lane == 1) | (lane == 2)
        assert bad[~touched].sum().item() == 0 and bad.double().mean().item() > 0.45
    frac = bad[touched].double().mean().item()
    print(f"planted defect '{defect}', seed {seed:#x}: {100 * frac:.2f} % of the touched elements rejected")
    assert frac > 0.9


# ---------------------------------------------------------------------------------------- stream addressing in the consumers

B_, C_, HW_, LDC_ = 3, 5, 100, 8  # two tiles per image, the second partial (36 pixels); C < ldc


def _inputs(dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B_, C_, HW_, generator=g).to(DEV)
    musig = (torch.rand(B_, 2, generator=g) + 0.1).to(DEV)
    y = torch.randn(B_ * HW_, LDC_, generator=g).to(TD[dt]).to(DEV)
    return x, musig, y


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_input_conversions_address_the_dense_stream(dt):
    """x_t = mu x + sigma eps[(b C + c) HW + pixel] with eps the float64 stream: c2w_nchw_to_nhwc_noise, and c2w_windows_to_nhwc_noise on
    shuffled, overlapping windows of a dataset array, which must give the bits of the dense conversion of the gathered batch"""
    seed = MIXED + dt
    x, musig, _ = _inputs(dt, 11)
    eps = N.eps_nchw(B_, C_, HW_, seed, DEV)
    want = N.xt_rows(x, eps, musig, dt, N.STREAM_TOL)
    y = torch.full((B_ * HW_, LDC_), 7.0, dtype=TD[dt], device=DEV)
    assert ops.nchw_to_nhwc_noise(x, seed, musig, y, B_, C_, HW_, LDC_, dt)
    R.report(f"nchw_to_nhwc_noise vs float64 stream {TD[dt]}", R.assert_within(y[:, :C_], want, what="nchw_to_nhwc_noise"))
    assert (y[:, C_:] == 0).all()
    for name, kw in (("seed + 1", dict(seed=seed + 1)), ("counter one block ahead", dict(seed=seed, block_shift=1)),
                     ("lanes 1 and 2 swapped", dict(seed=seed, lanes=(0, 2, 1, 3)))):
        wrong = N.xt_rows(x, N.eps_nchw(B_, C_, HW_, kw.pop("seed"), DEV, **kw), musig, dt, N.STREAM_TOL)
        R.assert_rejects(y[:, :C_], wrong, what=f"nchw_to_nhwc_noise, {name}")
    # a stream addressed per image (b C HW forgotten) or per plane would pass none of this: image 1's reference with image 0's noise
    wrong = N.xt_rows(x, eps.roll(1, 0), musig, dt, N.STREAM_TOL)
    R.assert_rejects(y[:, :C_], wrong, what="nchw_to_nhwc_noise, images' noise exchanged")
    # windows: frames of HW floats, a window = C consecutive frames; windows 4, 0, 2 overlap and are out of order
    data = torch.randn(9 * HW_, generator=torch.Generator().manual_seed(5)).to(DEV)
    off = torch.tensor([4 * HW_, 0, 2 * HW_], dtype=torch.int64, device=DEV)
    xg = torch.stack([data[o: o + C_ * HW_] for o in off.tolist()]).view(B_, C_, HW_).contiguous()
    yw = torch.full((B_ * HW_, LDC_), 7.0, dtype=TD[dt], device=DEV)
    yd = torch.full((B_ * HW_, LDC_), 7.0, dtype=TD[dt], device=DEV)
    assert ops.windows_to_nhwc_noise(data, off, seed, musig, yw, B_, C_, HW_, LDC_, dt)
    assert ops.nchw_to_nhwc_noise(xg, seed, musig, yd, B_, C_, HW_, LDC_, dt)
    assert torch.equal(yw, yd)
    R.report(f"windows_to_nhwc_noise vs float64 stream {TD[dt]}",
             R.assert_within(yw[:, :C_], N.xt_rows(xg, eps, musig, dt, N.STREAM_TOL), what="windows_to_nhwc_noise"))
    assert (yw[:, C_:] == 0).all()


def _loss_sum_bound(y, eps, tol):
    """fp64_ref.mse_loss_sum on the float64 stream, plus what an eps within tol of it moves the sum by: sum 2 |d| tol + tol^2"""
    s = R.mse_loss_sum(y, eps, B_, C_, HW_, LDC_)
    d = (R._rows(y, B_ * HW_, LDC_)[:, :C_].to(R.D) - N._to_rows(eps)).abs()
    return R.V(s.v, s.e + (2 * d * tol + tol * tol).sum() * (1 + 2 * R.U32))


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_loss_kernels_address_the_dense_stream(dt):
    seed = MIXED ^ (dt << 40)
    _, _, y = _inputs(dt, 12)
    eps = N.eps_nchw(B_, C_, HW_, seed, DEV)
    gscale = 0.37
    dy = torch.full((B_ * HW_, LDC_), 7.0, dtype=TD[dt], device=DEV)
    ls = torch.zeros(1, device=DEV)
    assert ops.mse_loss_grad_noise(y, seed, dy, ls, B_, C_, HW_, LDC_, gscale, dt)
    want = N.mse_dy_rows(y, eps, B_, C_, HW_, LDC_, gscale, dt, N.STREAM_TOL)
    R.report(f"mse_loss_grad_noise dy vs float64 stream {TD[dt]}", R.assert_within(dy[:, :C_], want, what="mse_loss_grad_noise dy"))
    assert (dy[:, C_:] == 0).all()
    R.report(f"mse_loss_grad_noise loss vs float64 stream {TD[dt]}",
             R.assert_within(ls, _loss_sum_bound(y, eps, N.STREAM_TOL), what="mse_loss_grad_noise loss"))
    out = torch.full((B_, C_, HW_), 7.0, device=DEV)
    ls2 = torch.zeros(1, device=DEV)
    assert ops.sq_err(y, seed, out, ls2, B_, C_, HW_, LDC_, dt)
    R.report(f"sq_err(seed) vs float64 stream {TD[dt]}",
             R.assert_within(out, N.sq_err_planes(y, eps, B_, C_, HW_, LDC_, N.STREAM_TOL), what="sq_err(seed)"))
    R.report(f"sq_err(seed) loss vs float64 stream {TD[dt]}",
             R.assert_within(ls2, _loss_sum_bound(y, eps, N.STREAM_TOL), what="sq_err(seed) loss"))
    for name, kw in (("seed ^ (1 << 32)", dict(seed=seed ^ (1 << 32))), ("counter one block ahead", dict(seed=seed, block_shift=1)),
                     ("cos and sin swapped", dict(seed=seed, swap_trig=True))):
        bad = N.eps_nchw(B_, C_, HW_, kw.pop("seed"), DEV, **kw)
        R.assert_rejects(dy[:, :C_], N.mse_dy_rows(y, bad, B_, C_, HW_, LDC_, gscale, dt, N.STREAM_TOL), what=f"mse dy, {name}")
        R.assert_rejects(out, N.sq_err_planes(y, bad, B_, C_, HW_, LDC_, N.STREAM_TOL), what=f"sq_err, {name}")
    R.assert_rejects(out, N.sq_err_planes(y, eps.roll(1, 1), B_, C_, HW_, LDC_, N.STREAM_TOL), what="sq_err, planes' noise exchanged")
