"""GPU checks of the window-streamed exact guidance: its four kernels (csrc/sampler.hip: c2w_window_gather_list, c2w_guidance_delta,
c2w_window_cotangent_list, c2w_window_grad_fold_list) against torch and the existing kernels, and the route
(score_fn.py::_guided_exact_streamed) against the autograd route and the imported reference's trajectories."""
import os

import numpy as np
import pytest
import torch

from climate2weather_amd import ops
from climate2weather_amd.ops import DTYPE_BF16, DTYPE_F16, DTYPE_F32
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.score_fn import BatchedScoreFunction, PoolStrideOperator, exact_window_list

pytestmark = pytest.mark.gpu

TINY = dict(embedding_dim=64, hidden_channels=[32, 64], hidden_blocks=[1, 1], attention_levels=[1], kernel_size=3, padding_mode="zeros")
WIDE = dict(TINY, hidden_channels=[64, 128])  # the smallest widths the 16-bit kernels take
DEFAULT = dict(embedding_dim=512, hidden_blocks=[3] * 5, hidden_channels=[128, 128, 256, 384, 512], kernel_size=3, padding_mode="zeros",
               attention_levels=[4])
TD = {DTYPE_F32: torch.float32, DTYPE_BF16: torch.bfloat16, DTYPE_F16: torch.float16}
DEV = "cuda:0"


def _golden(golden_dir, name):
    return {k: v for k, v in np.load(os.path.join(golden_dir, name), allow_pickle=False).items()}


def _lists(L, k):
    """A first window, interior windows and a last window from each of two members; -> (first, kind) host lists."""
    nwin = L - 2 * k
    per_member = [[0, 2, 3, nwin - 1], [0, 1, nwin - 1]]
    first = [m * L + i for m, wins in enumerate(per_member) for i in wins]
    kind = [(1 if i == 0 else 0) | (2 if i == nwin - 1 else 0) for wins in per_member for i in wins]
    return first, kind


def _dev_list(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dtype", [DTYPE_F32, DTYPE_BF16, DTYPE_F16])
@pytest.mark.parametrize("ldc", [64, 128])
@pytest.mark.parametrize("HW", [64, 1024])
@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("F", [2, 4])
def test_list_kernels_against_torch(F, k, HW, ldc, dtype):
    w = 2 * k + 1
    L, M, t_step = w + 5, 2, 2
    nobs = (L + t_step - 1) // t_step - 1  # the last observable frame is NOT observed: the truncation rule is exercised
    first, kind = _lists(L, k)
    n = len(first)
    fd, kd = _dev_list(first), _dev_list(kind)
    gen = torch.Generator(device=DEV).manual_seed(F * 1000 + k * 100 + HW + ldc + dtype)
    x = torch.randn((M, L, F, HW), device=DEV, generator=gen)

    # gather: bit-equal to the existing gather window by window, padding channels zero
    y = torch.full((n * HW, ldc), float("nan"), dtype=TD[dtype], device=DEV)
    ops.window_gather_list(x, y, fd, n, F, HW, k, ldc, dtype)
    yref = torch.full_like(y, float("nan"))
    for j, f0 in enumerate(first):
        ops.window_gather(x[f0 // L], yref[j * HW:], 1, F, HW, k, f0 % L, ldc, dtype)
    assert torch.equal(y, yref) and not y[:, w * F:].any()
    # ... and for a contiguous list, to one launch of it
    nwin = L - 2 * k
    yc = torch.full((nwin * HW, ldc), float("nan"), dtype=TD[dtype], device=DEV)
    ops.window_gather_list(x, yc, _dev_list([L + i for i in range(nwin)]), nwin, F, HW, k, ldc, dtype)
    ycref = torch.full_like(yc, float("nan"))
    ops.window_gather(x[1], ycref, nwin, F, HW, k, 0, ldc, dtype)
    assert torch.equal(yc, ycref)

    # cotangent: delta on the kept, observed slots -- as the existing gather casts it -- and zero everywhere else
    delta = torch.randn((M, nobs, F, HW), device=DEV, generator=gen)
    dense = torch.zeros((n, w, F, HW), device=DEV)
    placed = 0
    for j, (f0, kd_j) in enumerate(zip(first, kind)):
        m, i0 = divmod(f0, L)
        for tau in range(w):
            kept = tau == k or (tau < k and kd_j & 1) or (tau > k and kd_j & 2)
            frame = i0 + tau
            if kept and frame % t_step == 0 and frame // t_step < nobs:
                dense[j, tau] = delta[m, frame // t_step]
                placed += 1
    assert placed >= 4
    dyref = torch.full((n * HW, ldc), float("nan"), dtype=TD[dtype], device=DEV)
    ops.window_gather(dense.view(n * w, F, HW), dyref, 1, F, HW, k, 0, ldc, dtype)  # rows of window j: frames j w .. j w + w - 1
    for j in range(1, n):
        ops.window_gather(dense.view(n * w, F, HW), dyref[j * HW:], 1, F, HW, k, j * w, ldc, dtype)
    dy = torch.full_like(dyref, float("nan"))
    ops.window_cotangent_list(delta, dy, fd, kd, n, L, F, HW, k, t_step, nobs, ldc, dtype)
    assert torch.equal(dy, dyref) and not dy[:, w * F:].any()

    if ldc != 64 or dtype != DTYPE_F32:
        return  # the fold is fp32 whatever the network computes in, and has no row stride: once per (F, k, HW)
    # fold: inside the float64 bound of at most w fp32 additions, the scale and the add onto out; identical bits on two launches
    dx = torch.randn((n, w * F, HW), device=DEV, generator=gen)
    out0 = torch.randn((M * L, F, HW), device=DEV, generator=gen)
    scale = -0.375
    l0, nl = 1, M * L - 2  # frames 0 and M L - 1 are outside the launch
    ref = out0.double()
    mag = out0.double().abs()
    touched = torch.zeros(M * L, dtype=torch.bool)
    for l in range(l0, l0 + nl):
        terms = [dx[j].view(w, F, HW)[l - f0].double() for j, f0 in enumerate(first) if 0 <= l - f0 < w]
        if terms:
            touched[l] = True
            ref[l] += scale * torch.stack(terms).sum(0)
            mag[l] += abs(scale) * torch.stack(terms).abs().sum(0)
    outs = []
    for _ in range(2):
        out = out0.clone()
        ops.window_grad_fold_list(dx, out, fd, n, l0, nl, F, HW, k, scale)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    bound = (w + 2) * 2.0 ** -24 * mag
    assert ((outs[0].double() - ref).abs() <= bound).all()
    assert touched.any() and not touched.all() and torch.equal(outs[0][~touched.to(DEV)], out0[~touched.to(DEV)])
    assert not torch.equal(outs[0][touched.to(DEV)], out0[touched.to(DEV)])


@pytest.mark.parametrize("per_variable", [False, True])
@pytest.mark.parametrize("F,H,s_step,t_step", [(2, 8, 4, 2), (4, 32, 8, 3), (4, 32, 16, 6)])
def test_guidance_delta_plus_eps_is_the_fused_guidance(F, H, s_step, t_step, per_variable):
    L = 14
    nobs = (L + t_step - 1) // t_step
    gen = torch.Generator(device=DEV).manual_seed(F + H + t_step)
    x = torch.randn((L, F, H, H), device=DEV, generator=gen)
    eps = torch.randn((L, F, H, H), device=DEV, generator=gen)
    yobs = torch.randn((nobs, F, H // s_step, H // s_step), device=DEV, generator=gen)
    stdv = torch.rand(F, device=DEV, generator=gen) + 0.1
    gamma = torch.rand(F, device=DEV, generator=gen) * 0.1 if per_variable else 0.013
    mu, sigma = 0.83, 0.57
    fused = eps.clone()
    ops.guidance(x, fused, yobs, stdv, nobs, F, H, H, s_step, t_step, mu, sigma, gamma)
    kept = eps.clone()
    delta = torch.full((nobs, F, H, H), float("nan"), device=DEV)
    ops.guidance_delta(x, eps, yobs, stdv, delta, nobs, F, H, H, s_step, t_step, mu, sigma, gamma)
    assert torch.equal(eps, kept)  # only read
    got = eps.clone()
    got[::t_step][:nobs] += delta
    assert torch.equal(got, fused) and not torch.equal(fused, eps)


# ------------------------------------------------------------------------------------------------ the route
def _tiny(cfg=TINY, channels=6, precision="fp32", seed=3):
    torch.manual_seed(seed)
    net = ScoreUNet(channels=channels, spatial=2, activation=torch.nn.SiLU, **cfg).to(DEV).eval().requires_grad_(False)
    net.precision = precision
    return net


@pytest.mark.parametrize("name,gvec", [("cond_c1_exact", False), ("cond_c1_gvec_exact", True)])
@pytest.mark.parametrize("fused", [True, False])
def test_golden_trajectories_through_the_streamed_route(golden_dir, name, gvec, fused):
    s, sg = _golden(golden_dir, "sampler.npz"), _golden(golden_dir, "sampler_gamma.npz")
    src = sg if gvec else s
    pipe = SDAPipeline()
    dev = torch.device(DEV)
    sf = BatchedScoreFunction(_tiny(), markov_order=1, batch_size=4, device=dev, noise_process=pipe)
    sf.exact_streamed = True
    sf.condition_on(A=PoolStrideOperator(8, 2), y=torch.from_numpy(s["y_obs"]), std=torch.from_numpy(s["std"]),
                    gamma=torch.from_numpy(sg["gamma"]) if gvec else float(s["gamma"]), exact_grad=True)
    assert sf._fused_guidance is None
    sf.device_resident = fused
    zs = [torch.from_numpy(z) for z in src[name + ".z"]]
    noise = torch.from_numpy(s["cond_c0.noise"] if gvec else s[name + ".noise"])
    xs = pipe.sample(sf, noise, steps=4, corrections=1, tau=0.5, device=dev if fused else torch.device("cpu"), show_progressbar=False,
                     z_draws=zs)
    ref = torch.from_numpy(src[name + ".x"])
    assert (xs.cpu() - ref).abs().max().item() <= 3e-4 * ref.abs().max().item()


def _scale_rel(a, b):
    return (a.double() - b.double()).abs().max().item() / b.double().abs().max().item()


def _both_routes(net, k, x, t, A, y, std, gamma, batch_size):
    """(streamed, autograd route) of one guided evaluation."""
    sf = BatchedScoreFunction(net, markov_order=k, batch_size=batch_size, device=torch.device(DEV), noise_process=SDAPipeline())
    sf.condition_on(A=A, y=y, std=std, gamma=gamma, exact_grad=True)
    sf.exact_streamed = True
    streamed = sf(x, t).clone()
    sf.exact_streamed = False
    return streamed, sf(x, t).clone()


def test_one_evaluation_fp32_matches_the_autograd_route(golden_dir):
    s = _golden(golden_dir, "sampler.npz")
    x = torch.from_numpy(s["score_x"]).to(DEV)
    streamed, autograd = _both_routes(_tiny(), 1, x, torch.tensor(0.7), PoolStrideOperator(8, 2), torch.from_numpy(s["y_obs"]),
                                      torch.from_numpy(s["std"]), float(s["gamma"]), 4)
    print("fp32 streamed vs autograd route, scale-relative:", _scale_rel(streamed, autograd))
    assert _scale_rel(streamed, autograd) <= 1e-4  # the project's fp32 parity bound
    sf0 = BatchedScoreFunction(_tiny(), markov_order=1, batch_size=4, device=torch.device(DEV), noise_process=SDAPipeline())
    sf0.condition_on(A=PoolStrideOperator(8, 2), y=torch.from_numpy(s["y_obs"]), std=torch.from_numpy(s["std"]), gamma=float(s["gamma"]),
                     exact_grad=False)
    assert _scale_rel(sf0(x, torch.tensor(0.7)), streamed) > 1e-2  # the network term is there


_FP32_REF = {}


def _case(which):
    """(cfg, F, k, L, H, s_step, t_step) and the fp32 autograd-route result, computed once and shared by the 16-bit cases."""
    cfg, F, k, L, H, s_step, t_step = (WIDE, 2, 1, 9, 32, 8, 2) if which == "wide" else (DEFAULT, 4, 6, 25, 32, 16, 6)
    if which not in _FP32_REF:
        gen = torch.Generator(device=DEV).manual_seed(11)
        A = PoolStrideOperator(s_step, t_step)
        truth = torch.randn((L, F, H, H), device=DEV, generator=gen) * 0.5
        x = torch.randn((L, F, H, H), device=DEV, generator=gen)
        y = A(truth)
        std = torch.full((1, F, 1, 1), 0.2)
        net = _tiny(cfg, channels=F * (2 * k + 1))
        _, ref = _both_routes(net, k, x, torch.tensor(0.6), A, y, std, 1e-2, 4)
        _FP32_REF[which] = (x, A, y, std, ref)
    return (cfg, F, k) + _FP32_REF[which]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("which", ["wide", "default"])
def test_16_bit_streamed_is_as_close_to_fp32_as_the_autograd_route(which, precision):
    """Both routes in 16 bit against the autograd route in fp32: the streamed route draws other roundings of the same arithmetic, so
    its error may be up to twice the other's maximum, not more."""
    cfg, F, k, x, A, y, std, ref = _case(which)
    if which == "default":
        assert exact_window_list(1, 25, 6, 6, y.shape[0])[0] == [0, 6, 12]
    net = _tiny(cfg, channels=F * (2 * k + 1), precision=precision)
    streamed, autograd = _both_routes(net, k, x, torch.tensor(0.6), A, y, std, 1e-2, 4)
    es, ea = _scale_rel(streamed, ref), _scale_rel(autograd, ref)
    print(f"{which} {precision}: err(streamed) = {es:.3e}, err(autograd route) = {ea:.3e}, ratio = {es / ea:.3f}")
    assert torch.isfinite(streamed).all() and ea > 0
    assert es <= 2 * ea


def test_peak_memory_is_below_the_autograd_route():
    L, F, H, k = 200, 2, 32, 1
    gen = torch.Generator(device=DEV).manual_seed(2)
    A = PoolStrideOperator(8, 6)
    truth = torch.randn((L, F, H, H), device=DEV, generator=gen)
    x = torch.randn((L, F, H, H), device=DEV, generator=gen)
    sf = BatchedScoreFunction(_tiny(), markov_order=k, batch_size=16, device=torch.device(DEV), noise_process=SDAPipeline())
    sf.condition_on(A=A, y=A(truth), std=0.2, gamma=1e-2, exact_grad=True)
    peaks = {}
    for mode in (True, False, True):  # the streamed route first and last: neither order favours it
        sf.exact_streamed = mode
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = sf(x, torch.tensor(0.6))
        torch.cuda.synchronize()
        peaks.setdefault(mode, []).append(torch.cuda.max_memory_allocated() - base)
        del out
    print("peak bytes above the resident state: streamed", peaks[True], "autograd route", peaks[False])
    assert max(peaks[True]) < peaks[False][0]
