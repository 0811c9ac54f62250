"""The spectrum kernel on the MI355X (csrc/spectrum.hip through ops.rapsd and spectra.rapsd): every size, field kind and batch shape
against the float64 definition by the rule of tests/fp64_spectrum_ref.py -- a spectrum passes if its error is at most four times the
larger of the fp32 vendor transform's error on the same field and 16 * 2^-24 -- then the properties the interface promises: the same
bits wherever a field lies in the batch, nothing written past n_fields, nothing written for an unsupported shape."""
import numpy as np
import pytest
import torch

import fp64_spectrum_ref as R
from climate2weather_amd import ops, spectra

pytestmark = pytest.mark.gpu

SIZES = (8, 16, 32, 64, 128)
CANARY = -7.25


def dev():
    return torch.device("cuda:0")


def counts(N):
    """field counts: at N <= 32 a workgroup holds 16, 8 or 4 fields -- 1 and 3 leave it partly empty, 257 ends in a partly empty one
    after more workgroups than N = 8 and 16 need; at N >= 64 a workgroup is a field"""
    return (1, 3, 257) if N <= 32 else (1, 5)


_CACHE = {}


def fields_and_reference(N):
    """(names, kinds, x (n, N, N) fp32, S64 (n, N/2), bound (n,)) -- computed once per size, shared and left unchanged"""
    if N not in _CACHE:
        dense, sparse = R.dense_fields(N), R.sparse_fields(N)
        names = list(dense) + list(sparse)
        x = np.stack(list(dense.values()) + list(sparse.values()))
        S64 = R.rapsd64(x)
        bound = np.array([R.bound_log(x[i], S64[i]) if n in dense else R.bound_abs(x[i], S64[i]) for i, n in enumerate(names)])
        _CACHE[N] = (names, [n in dense for n in names], x, S64, bound)
    return _CACHE[N]


def launch(x, n_fields=None, rows=None):
    """spec (rows, N/2) from ops.rapsd on the first n_fields of x, rows past them holding the canary"""
    n, N = x.shape[0], x.shape[-1]
    n_fields = n if n_fields is None else n_fields
    spec = torch.full((rows or n, N // 2), CANARY, dtype=torch.float32, device=x.device)
    assert ops.rapsd(x, spec, n_fields, N, N)
    return spec


def errors(S, names_dense, x, S64):
    return np.array([R.e_log(S[i], S64[i]) if d else R.e_abs(S[i], S64[i], x[i]) for i, d in enumerate(names_dense)])


@pytest.mark.parametrize("N", SIZES)
def test_every_field_kind_and_batch_shape_against_float64(N):
    names, dense, x, S64, bound = fields_and_reference(N)
    kinds = len(names)
    for n in counts(N):
        worst, bad = {}, []
        for start in range(0, kinds if n < kinds else 1, n):  # batches of n until every kind has been in one; at n = 257 the kinds cycle
            idx = (start + np.arange(n)) % kinds              # through the batch and every kind meets every slot of a workgroup
            S = launch(torch.as_tensor(x[idx]).to(dev())).cpu().numpy()
            e = errors(S, [dense[i] for i in idx], x[idx], S64[idx])
            for j, i in enumerate(idx):
                worst[names[i]] = max(worst.get(names[i], 0.0), e[j] / (bound[i] / R.FACTOR))
            bad += [(names[i], j, e[j], bound[i]) for j, i in enumerate(idx) if not e[j] <= bound[i]]
        print(f"N={N} n={n}: error over max(yardstick, floor), limit {R.FACTOR}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        assert len(worst) == kinds and not bad, bad[:5]


@pytest.mark.parametrize("N", SIZES)
def test_same_bits_at_every_position_and_on_every_call(N):
    names, dense, x, _, _ = fields_and_reference(N)
    n = 37 if N <= 32 else 5
    rng = np.random.default_rng(N)
    batch = rng.standard_normal((n, N, N)).astype(np.float32)
    probe = x[names.index("power_law")]
    spots = sorted({0, 1, n // 2, n - 2, n - 1})
    for s in spots:
        batch[s] = probe
    xb = torch.as_tensor(batch).to(dev())
    a, b = launch(xb), launch(xb)
    alone = launch(torch.as_tensor(probe[None]).to(dev()))
    assert torch.equal(a, b)
    for s in spots:
        assert torch.equal(a[s], alone[0]), s


@pytest.mark.parametrize("N,n,rows", [(8, 17, 40), (16, 9, 20), (32, 5, 12), (64, 2, 4), (128, 1, 3)])
def test_rows_past_n_fields_keep_their_canary(N, n, rows):
    x = torch.randn(rows, N, N, device=dev())  # fields past n_fields exist and must not be read into a result either
    spec = launch(x, n_fields=n, rows=rows)
    assert torch.isfinite(spec[:n]).all() and (spec[:n] >= 0).all()
    assert torch.equal(spec[n:], torch.full_like(spec[n:], CANARY))


@pytest.mark.parametrize("H,W", [(24, 20), (256, 256), (64, 32), (32, 64), (12, 12)])
def test_unsupported_shapes_answer_false_and_write_nothing(H, W):
    assert not ops.rapsd_supported(H, W)
    x = torch.randn(2, H, W, device=dev())
    spec = torch.full((2, max(H, W)), CANARY, dtype=torch.float32, device=dev())
    assert ops.rapsd(x, spec, 2, H, W) is False
    assert torch.equal(spec, torch.full_like(spec, CANARY))


def test_nan_field_gives_nan_spectrum_and_spares_its_neighbours():
    x = torch.randn(9, 16, 16, device=dev())
    x[4, 3, 3] = float("nan")
    S = spectra.rapsd(x)
    assert torch.isnan(S[4]).all() and torch.isfinite(S[:4]).all() and torch.isfinite(S[5:]).all()


def test_general_route_on_a_gpu_tensor():
    x = (0.5 + np.random.default_rng(24).standard_normal((3, 24, 20))).astype(np.float32)
    S64 = R.rapsd64(x)
    S = spectra.rapsd(torch.as_tensor(x).to(dev()), normalize=False)
    assert S.is_cuda and S.shape == (3, 12)
    e, b = R.e_log(S.cpu().numpy(), S64), R.bound_log(x, S64)
    print(f"24x20 on the device: e_log {e} bound {b}")
    assert np.all(e <= b)


def test_strided_half_precision_input_takes_the_kernel():
    base = torch.randn(2, 3, 32, 64, device=dev()).to(torch.float16)
    view = base[..., ::2]
    want = R.rapsd64(view.double().cpu().numpy(), normalize=True)
    got = spectra.rapsd(view)
    assert got.shape == (2, 3, 16) and got.dtype == torch.float32
    assert np.allclose(got.double().cpu().numpy(), want, rtol=1e-5)


def test_spectral_report_against_the_float64_reference():
    """(M, L, F) = (2, 5, 2) at 32 x 32 with an 8 x 8 obs.  Spectra by the rule above.  MELR: |log(a / b)| moves by at most the two
    spectra's log errors, and normalising adds at most each spectrum's largest relative error again, so a mean of such terms is within
    2 (bound_sample + bound_truth) of the float64 value -- with the bounds' maxima over the fields that enter it (the weighted mode adds
    the movement of its weights)."""
    M, L, F, N = 2, 5, 2, 32
    rng = np.random.default_rng(7)
    truth = np.stack([np.stack([R.power_law(N, 300 + 10 * l + f) + 0.3 for f in range(F)]) for l in range(L)]).astype(np.float32)
    samples = (truth[None] + 0.1 * rng.standard_normal((M, L, F, N, N))).astype(np.float32)
    obs = truth.reshape(L, F, 8, 4, 8, 4).mean(axis=(3, 5)).astype(np.float32)
    rep = spectra.spectral_report(torch.as_tensor(samples).to(dev()), torch.as_tensor(truth).to(dev()), torch.as_tensor(obs).to(dev()))
    for f, (name, v) in enumerate(rep):
        assert name == f"var{f}"
        for key, x in (("sample_rapsd_over_time", samples[:, :, f]), ("gt_rapsd_over_time", truth[:, f]), ("obs_rapsd_over_time", obs[:, f])):
            raw64 = R.rapsd64(x)
            want = raw64 / raw64.sum(-1, keepdims=True)
            b = R.bound_log(x.reshape(-1, *x.shape[-2:]), raw64.reshape(-1, raw64.shape[-1])).reshape(x.shape[:-2])
            got = v[key].double().cpu().numpy()
            assert got.shape == want.shape
            e = R.e_log(got, want)
            assert np.all(e <= 2 * b + 2.0 ** -23), (key, e.max(), b.max())  # normalising: the sum's error, and one fp32 rounding of S / sum
            if key == "sample_rapsd_over_time":
                bs = b.max()
            elif key == "gt_rapsd_over_time":
                bg = b.max()
        sr, gr = R.rapsd64(samples[:, :, f], normalize=True), R.rapsd64(truth[:, f], normalize=True)
        rmax = np.abs(np.log(sr / gr)).max()  # "weighted": the weights S_truth / sum move by 2 bg relative, on terms of at most rmax
        for mode, kw in (("mean", {}), ("weighted", dict(do_weighted=True)), ("max", dict(do_max=True))):
            got = v["melr"][mode].cpu().numpy()
            want = R.melr_reference(sr, gr, **kw)
            tol = 2 * (bs + bg) + 2.0 ** -22 + (2 * bg * rmax if mode == "weighted" else 0.0)
            print(f"{name} melr {mode}: {got} vs {want}, tolerance {tol:.3g}")
            assert got.shape == (M,) and np.all(np.abs(got - want) <= tol), (mode, got, want, tol)
        assert v["obs_rapsd_over_time"].shape == (L, 4) and v["obs_wavelengths"].shape == (4,)
        assert float(v["obs_wavelengths"][1]) == pytest.approx(6.0 * 4 * 8)
